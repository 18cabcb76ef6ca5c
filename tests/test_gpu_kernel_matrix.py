"""Every case of tests/kernel_matrix.py against the oracle: each compiled form of the step and rollout kernels (A, LIGHTS, OBS,
BIG, WAVES, MAG, role split, wavefronts per env) and of the A-templated operators, bit for bit, on worlds where episodes end,
egos collide or leave the road and - with lights - run red lights.  Plus both sides of the batch-size dispatch edges, at thresholds
read from the device's CU count, and the rollout's batch chunking with a partial last chunk.

The cases are grouped by (world, A, LIGHTS, edge): the oracle runs once per group - on slices of the batch (the first envs, the
envs on either side of each cut, the last envs, with cfg.env_base = lo) when the batch is large - and every case advances a device
state of its own with the same actions.  A rollout is compared with the oracle's repeated steps (tde_oracle_env_rollout is
those steps: tests/test_oracle_properties.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import oracle  # noqa: E402
from tests import kernel_matrix as km  # noqa: E402
from tests.test_gpu_parity import assert_state_equal, dev, random_agents  # noqa: E402
from torchdriveenv_amd import _abi, _lib, ops  # noqa: E402
from torchdriveenv_amd.state import EnvState  # noqa: E402
from torchdriveenv_amd.synth import synthetic_town, synthetic_world  # noqa: E402

DEV = "cuda:0"
T = 30                  # steps per group (max_steps 20: every env re-spawns at least once); the whole state is compared after
                        # the steps of _check_steps(T)
AGENT_KEYS = set(_abi.STATE_AGENT_F32 + _abi.STATE_AGENT_I32 + _abi.STATE_AGENT_U8)
CACHE_KEYS = {"slot_cache", "env_cache", "act_cache"}
GROUPS = km.groups()
_WORLDS = {}


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _world(kind, A):
    """one world per (kind, A) for the module.  Both kinds are signalised; their stop lines are lengthened along the lane (25 m /
    60 m half-length instead of 0.5 m) so that within a few dozen steps some egos stand on a red one: every lit group sees light
    terminations.  Oracle and kernels read the same table."""
    if (kind, A) not in _WORLDS:
        if kind == "town":
            w = synthetic_town(n_scn=4, A=A, n_streets=4, spacing=100.0, ext=160.0, min_gap=3.4, n_signals=4)
            assert w.ints["hints"] & _abi.WORLD_LARGE_GRID
            w.arrays["stoplines"]["hl"][:] = 25.0
        else:
            w = synthetic_world(n_scn=8, A=A, seed=A, n_maps=2)
            assert not w.ints["hints"] & _abi.WORLD_LARGE_GRID
            w.arrays["stoplines"]["hl"][:] = 60.0
        assert w.has_lights
        _WORLDS[(kind, A)] = (w, w.to_device(DEV))
    return _WORLDS[(kind, A)]


def _slices(B, cuts):
    """[lo, hi) ranges the oracle runs: the whole batch when it is small, else the first 16 envs, 8 on either side of each cut
    and the last 8"""
    if not cuts:
        return [(0, B)]
    r = [(0, 16)] + [(max(0, c - 8), min(B, c + 8)) for c in cuts] + [(B - 8, B)]
    out = []
    for lo, hi in sorted(r):
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def _check_steps(T):
    return (0, 2, T - 1)


def _actions(B, seed, T=T):
    """[T, B, 2]: half the egos drive on steadily (they reach the stop lines), half swerve (offroad, collisions)"""
    rng = np.random.default_rng(seed)
    careful = (np.arange(B) % 2) == 0
    acc = np.where(careful, rng.uniform(0.6, 1.0, (T, B)), rng.uniform(-0.3, 1.0, (T, B)))
    steer = np.where(careful, rng.uniform(-0.02, 0.02, (T, B)), rng.uniform(-0.3, 0.3, (T, B)))
    return np.stack([acc, steer], -1).astype(np.float32)


def _cut(arrays, A, lo, hi, skip=()):
    """the envs [lo, hi) of a state's arrays, flat"""
    out = {}
    for k, a in arrays.items():
        if a is None or k in skip or k in CACHE_KEYS or k == "action":
            continue
        a = a.reshape(-1)
        if k in AGENT_KEYS:
            out[k] = a[lo * A:hi * A]
        else:
            per = a.size // (arrays["scn"].size)
            out[k] = a[lo * per:hi * per]
    return out


class _Oracle:
    """the oracle on slices of the batch: per step the rewards, done bits, magnitudes; the whole state after the check steps
    (of a run of T steps: the first, the third and the last)"""

    def __init__(self, cfg, world, A, slices, actions, T=T):
        self.slices, self.A, self.T, self.check = slices, A, T, _check_steps(T)
        self.reward = np.zeros((T, actions.shape[1]), np.float32)
        self.done = np.zeros((T, actions.shape[1]), np.uint8)
        self.mag = np.zeros((T, actions.shape[1], 4), np.float32)
        self.reset, self.snap = {}, {t: {} for t in self.check}
        for lo, hi in slices:
            c = _abi.TdeConfig.from_buffer_copy(cfg)
            c.env_base = lo
            hs = EnvState(hi - lo, A)
            oracle.env_reset(c, world, hs)
            self.reset[lo] = hs.host()
            for t in range(T):
                hs["action"][...] = actions[t, lo:hi]
                oracle.env_step(c, world, hs)
                self.reward[t, lo:hi], self.done[t, lo:hi], self.mag[t, lo:hi] = hs["reward"], hs["done_bits"], hs["magnitudes"]
                if t in self.check:
                    self.snap[t][lo] = hs.host()

    def events(self):
        d = np.concatenate([self.done[:, lo:hi] for lo, hi in self.slices], 1)
        return int(((d & 1) != 0).sum()), int(((d & 12) != 0).sum()), int(((d & 16) != 0).sum())

    def check_state(self, host, t, where, skip=()):
        for lo, hi in self.slices:
            want = _cut(self.snap[t][lo] if t is not None else self.reset[lo], self.A, 0, hi - lo, skip)
            got = _cut(host, self.A, lo, hi, skip)
            assert_state_equal({k: v for k, v in want.items() if k in got}, got, f"{where}, envs [{lo}, {hi}), step {t}")

    def check_step(self, t, reward, done, where, mag=None):
        for lo, hi in self.slices:
            assert np.array_equal(reward[lo:hi].view(np.uint32), self.reward[t, lo:hi].view(np.uint32)), f"reward: {where} [{lo}, {hi}) step {t}"
            assert np.array_equal(done[lo:hi], self.done[t, lo:hi]), f"done bits: {where} [{lo}, {hi}) step {t}"
            if mag is not None:
                assert np.array_equal(mag[lo:hi].view(np.uint32), self.mag[t, lo:hi].view(np.uint32)), f"magnitudes: {where} [{lo}, {hi}) step {t}"


def _step_case(c, cfg, dw, B, A, acts, want, T=T):
    where = c.id()
    d = EnvState(B, A, device=DEV, with_obs=c.obs, with_magnitudes=c.mag, with_cache=c.cache)
    ops.env_reset(cfg, dw, d)
    want.check_state(d.host(), None, where + " (reset)")
    post = c.entry == "post_step"
    cfg_na = _abi.TdeConfig.from_buffer_copy(cfg)
    cfg_na.flags &= ~_abi.F_AUTORESET
    mag2 = torch.zeros(B, 4, device=DEV) if post else None
    _lib.kernel_override(step=c.form)
    try:
        for t in range(T):
            if post:                               # step without TDE_F_AUTORESET + tde_env_post_step == the one-launch step
                ops.env_step(cfg_na, dw, d, action=acts[t])
                ops.env_post_step(cfg, dw, d, mag2)
            else:
                ops.env_step(cfg, dw, d, action=acts[t])
            mag = mag2 if post else d["magnitudes"]
            want.check_step(t, d["reward"].cpu().numpy(), d["done_bits"].cpu().numpy(), where,
                            None if mag is None else mag.cpu().numpy())
            if t in _check_steps(T):
                want.check_state(d.host(), t, where, skip=("magnitudes",))
                if c.obs:
                    got, ref = d["obs"], ops.state_obs(dw, d)
                    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), f"obs != tde_state_obs: {where} step {t}"
    finally:
        _lib.kernel_override()


def _rollout_case(c, cfg, dw, B, A, acts, want, T=T):
    where = c.id()
    d = EnvState(B, A, device=DEV, with_episode=False, with_magnitudes=False)
    ops.env_reset(cfg, dw, d)
    _lib.kernel_override(rollout=c.form)
    try:
        r, dn = ops.env_rollout(cfg, dw, d, acts)
        torch.cuda.synchronize()
    finally:
        _lib.kernel_override()
    r, dn = r.cpu().numpy(), dn.cpu().numpy()
    for t in range(T):
        want.check_step(t, r[t], dn[t], where)
    # (the Monitor statistics, done_bits and magnitudes belong to the closed-loop step: a rollout leaves them alone)
    want.check_state(d.host(), T - 1, where, skip=("done_bits", "magnitudes", "ep_return", "ep_final", "ep_final_len"))


def _operator_case(c, B, A):
    rng = np.random.default_rng(100 + A)
    ag = random_agents(rng, B, A, spread=2.0 + A * 0.8)
    args = [ag[k] for k in ("x", "y", "psi", "length", "width", "present")]
    if c.entry == "collide":
        want = oracle.compute_collision(B, A, *args)
        got = ops.compute_collision(B, A, *map(dev, args)).cpu().numpy()
    else:
        act = np.stack([rng.uniform(-1, 1, B * A), rng.uniform(-0.3, 0.3, B * A)], -1).astype(np.float32)
        h = {k: ag[k].copy() for k in ("x", "y", "psi", "v")}
        oracle.kinematics_step(h["x"], h["y"], h["psi"], h["v"], ag["lr"], ag["present"], act)
        want = oracle.compute_collision(B, A, h["x"], h["y"], h["psi"], ag["length"], ag["width"], ag["present"])
        d = {k: dev(ag[k]) for k in ("x", "y", "psi", "v", "lr", "length", "width", "present")}
        got = ops.kin_collide_step(B, A, d["x"], d["y"], d["psi"], d["v"], d["lr"], d["length"], d["width"], d["present"],
                                   dev(act)).cpu().numpy()
        for k in ("x", "y", "psi", "v"):
            assert np.array_equal(d[k].cpu().numpy().view(np.uint32), h[k].view(np.uint32)), f"{k}: {c.id()}"
    assert np.array_equal(got, want), c.id()
    if A > 1:
        assert 0 < want.sum() < want.size, c.id()              # both outcomes


@pytest.mark.parametrize("key", list(GROUPS), ids=["-".join(map(str, k)).strip("-") for k in GROUPS])
def test_every_kernel_form_matches_the_oracle(key):
    kind, A, lights, edge = key
    cases = GROUPS[key]
    cu = _cu()
    B = cases[0].B(cu)
    world, dw = _world(kind, A)
    flags = _abi.F_ALL | (_abi.F_TRAFFIC_LIGHTS if lights else 0)
    cfg = _abi.default_config(seed=1000 + 16 * A + 2 * lights + (kind == "town"), flags=flags, max_steps=20, distance_cutoff=0.25)
    cuts = tuple(sorted({x for c in cases for x in c.cuts(cu)}))
    acts_h = _actions(B, seed=A + 7 * lights)
    want = _Oracle(cfg, world, A, _slices(B, cuts), acts_h)
    n_end, n_hit, n_red = want.events()
    assert n_end > 0 and n_hit > 0 and (n_red > 0 or not lights), (key, n_end, n_hit, n_red)      # nothing passes vacuously
    acts = dev(acts_h)
    # (the gap cache first: the step and rollout cases after it read what it filled)
    for c in sorted(cases, key=lambda c: c.entry != "first_gaps"):
        assert c.B(cu) == B
        if c.entry == "first_gaps":
            fg = dw.tensors["first_gap"].view(torch.int32)
            fg.zero_()
            ops.first_gaps(cfg, dw)
            torch.cuda.synchronize()
            # keyed entries for every NPC slot of every scenario (slot 0, the ego, has none: at A = 1 there is nothing to fill)
            keyed = (fg.view(world.n_scn, A, 2)[:, :, 1] != 0).cpu().numpy()
            assert not keyed[:, 0].any() and keyed[:, 1:].all(), c.id()
        elif c.entry in ("collide", "kin_collide"):
            _operator_case(c, B, A)
        elif c.entry == "rollout":
            _rollout_case(c, cfg, dw, B, A, acts, want)
        else:
            _step_case(c, cfg, dw, B, A, acts, want)

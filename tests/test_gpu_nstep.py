"""The n-step sample on the GPU (include/tde_nstep.h; ReplayBuffer.sample_nstep).  Nothing here has a tolerance: every output is held bit
for bit to the numpy restatement (tests/nstep_ref.py) - through the C-ABI on rings filled by hand (tests/ring_util.HandRing) with the
history of tests/nstep_cases.py, whose stop reasons tests/test_nstep_cpu.py vouches for, with canaries around every output - and to the
one-step samplers where the contract says the two agree."""
import numpy as np
import pytest
import torch

from tests import nstep_cases as K
from tests import nstep_ref as N
from tests import replay_ref as R
from tests import ring_util as U
from tests import terminal_ref as T
from tests.ring_util import bits, guarded, guards_ok
from torchdriveenv_amd import ops
from torchdriveenv_amd.config import EnvConfig, RendererConfig, SimulatorConfig, VectorObs
from torchdriveenv_amd.env import BatchedWaypointEnv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = U.FIELDS + ("discounts", "steps")


def outputs(ring, n):
    obs = ((n, 3 * ring.n_stack, ring.plane), torch.uint8) if ring.plane else ((n, ring.D), torch.float32)
    spec = {"observations": obs, "next_observations": obs, "actions": ((n, 2), torch.float32), "rewards": ((n,), torch.float32),
            "dones": ((n,), torch.uint8), "indices": ((n, 2), torch.int32), "discounts": ((n,), torch.float32), "steps": ((n,), torch.uint8)}
    whole, out = {}, {}
    for k, (shape, dt) in spec.items():
        whole[k], out[k] = guarded(shape, dt, DEV)
    return whole, out


def run_nstep(ring, n_steps, gamma, pool, pairs=None, n=None, seed=0, draw=0):
    """tde_nstep_sample of the given pairs, or of n drawn ones, into guarded outputs -> numpy arrays (the canaries checked)"""
    n = len(pairs) if pairs is not None else n
    whole, out = outputs(ring, n)
    tin = None if pairs is None else torch.from_numpy(np.asarray(pairs, np.int32).reshape(-1, 2)).to(DEV)
    ops.nstep_sample(ring.rp, ring.tm if pool else None, DEV, ring.first, ring.count, n, n_steps, gamma, out, tin, seed, draw)
    for k in FIELDS:
        assert guards_ok(whole[k], out[k]), k
    return {k: out[k].cpu().numpy() for k in FIELDS}


def check_nstep(ring, n_steps, gamma, pool, pairs=None, n=None, seed=0, draw=0):
    got = run_nstep(ring, n_steps, gamma, pool, pairs, n, seed, draw)
    idx = ring.ref.draw(seed, draw, n) if pairs is None else pairs
    want = N.gather(ring.ref, idx, n_steps, gamma, terminal=pool)
    for k in FIELDS:
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), (k, n_steps, gamma, pool)
    return got


def settings(cheap):
    """(n_steps, gamma): all of them where the stacks are small, every n_steps and every gamma once where they are not"""
    if cheap:
        return [(n, g) for n in K.N_STEPS for g in K.GAMMAS]
    return list(zip(K.N_STEPS, (0.99, 0.5, 1.0, 0.0))) + [(5, 0.99)]


# ---- 1. the history of every stop reason, at every shape ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,plane", K.PLANES)
def test_planes_against_the_restatement(ns, plane):
    ring = K.history_ring(ns, plane=plane, dev=DEV)
    assert ring.check_state() == (6, 5, 11)
    pairs = ring.stored_pairs()
    for pool in (False, True):
        for n_steps, gamma in settings(plane == 16):
            got = check_nstep(ring, n_steps, gamma, pool, pairs)
            assert got["steps"].min() >= 1 and got["steps"].max() == min(n_steps, ring.count)
    ring.check_state()                                      # the call reads the ring


@pytest.mark.parametrize("D", K.ROWS)
def test_rows_against_the_restatement(D):
    ring = K.history_ring(D=D, dev=DEV)
    assert ring.check_state() == (6, 5, 11)
    pairs = ring.stored_pairs()
    for pool in (False, True):
        for n_steps, gamma in settings(True):
            check_nstep(ring, n_steps, gamma, pool, pairs)
        for n in (1, 3, 4, 5):                              # four samples per workgroup: a last workgroup that is not full
            check_nstep(ring, 5, 0.99, pool, pairs[7:7 + n])
    ring.check_state()


def test_the_stated_order_is_not_a_fused_multiply_add():
    ring = K.history_ring(D=5, dev=DEV)
    pairs = ring.stored_pairs()
    got = check_nstep(ring, 5, 0.99, False, pairs)
    fused = np.array([K.fused_sum([ring.ref.reward[(s + k) % ring.C, e] for k in range(m)], 0.99)[0]
                      for (s, e), m in zip(pairs, got["steps"])], np.float32)
    assert (bits(got["rewards"]) != bits(fused)).any()


@pytest.mark.parametrize("shape", [dict(n_stack=8, plane=16), dict(n_stack=3, plane=16), dict(D=5)], ids=str)
def test_a_saturated_age_along_the_look_ahead(shape):
    ring = K.age_ring(dev=DEV, **shape)
    ring.check_state()
    assert (ring.t["age"][:, 0] == 255).all()
    pairs = ring.stored_pairs()
    for pool in (False, True):
        for n_steps in (5, 64):
            check_nstep(ring, n_steps, 0.99, pool, pairs)


def test_the_look_ahead_at_its_full_width():
    """n_steps = 64 where 64 stored steps lie ahead (C = 12 above never has them): endings in lane 63 and one beyond it, m = count - off
    = 64, and the newest step; tests/test_nstep_cpu.py::test_long_ring_reaches_the_full_width_of_the_look_ahead vouches for the pairs"""
    from tests import sequence_cases as S

    pairs = S.long_pairs()
    for pool in (False, True):
        ring = S.long_ring(pool=pool, dev=DEV)
        assert ring.check_state() == (0, 280, 280)
        got = check_nstep(ring, 64, 0.99, pool, pairs)
        assert got["steps"].max() == 64 and got["steps"].min() == 1 and 63 in got["steps"]
        check_nstep(ring, 64, 0.99, pool, pairs[1::2])      # env 1 alone: no ending anywhere


# ---- 2. pairs that gather zeros ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.INVALID_RINGS))
@pytest.mark.parametrize("mode", list(U.INVALID_MODES))
def test_invalid_pairs_gather_zeros_between_valid_ones(mode, name):
    case = U.INVALID_RINGS[name]
    ring = U.invalid_ring(mode, name, DEV)
    assert ring.check_state() == case["state"]
    pairs = np.array(U.interleaved(case), np.int32)
    bad = np.arange(len(pairs)) % 2 == 0
    for n in sorted({len(pairs), *U.INVALID_N}):
        for pool in (False, True):
            got = check_nstep(ring, 3, 0.99, pool, pairs[:n])
            b = bad[:n]
            assert np.array_equal(got["indices"], pairs[:n])
            for k in FIELDS:
                if k != "indices":
                    assert not bits(got[k][b]).any(), k
            for i in np.flatnonzero(~b):
                assert got["steps"][i] >= 1 and got["discounts"][i] > 0 and got["observations"][i].any(), i


# ---- 3. the drawn path --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.DRAW_CASES))
def test_the_draw_is_the_one_step_samplers(name):
    ring = U.draw_ring(name, DEV)
    ring.check_state()
    lists = []
    for draw in U.DRAWS:
        one, _ = ring.check_sample(n=U.DRAW_N, seed=U.DRAW_SEED, draw=draw)
        for pool in (False, True):
            got = check_nstep(ring, 3, 0.99, pool, n=U.DRAW_N, seed=U.DRAW_SEED, draw=draw)
            assert np.array_equal(got["indices"], one["indices"])
        lists.append(got["indices"].tobytes())
    assert len(set(lists)) == len(U.DRAWS)
    assert check_nstep(ring, 2, 0.5, True, n=1, seed=U.DRAW_SEED, draw=3)["indices"].shape == (1, 2)


# ---- 4. identities on the GPU alone ----------------------------------------------------------------------------------------------------------
def one_step_gpu(ring, pairs, pool):
    obs = ((len(pairs), 3 * ring.n_stack, ring.plane), torch.uint8) if ring.plane else ((len(pairs), ring.D), torch.float32)
    out = {"observations": torch.empty(*obs[0], dtype=obs[1], device=DEV), "next_observations": torch.empty(*obs[0], dtype=obs[1], device=DEV),
           "actions": torch.empty((len(pairs), 2), device=DEV), "rewards": torch.empty(len(pairs), device=DEV),
           "dones": torch.empty(len(pairs), dtype=torch.uint8, device=DEV), "indices": torch.empty((len(pairs), 2), dtype=torch.int32, device=DEV)}
    tin = torch.from_numpy(np.asarray(pairs, np.int32).reshape(-1, 2)).to(DEV)
    if pool:
        ops.terminal_sample(ring.rp, ring.tm, DEV, ring.first, ring.count, len(pairs), out, tin)
    else:
        ops.replay_sample(ring.rp, DEV, ring.first, ring.count, len(pairs), out, tin)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("shape", [dict(n_stack=3, plane=2304), dict(n_stack=8, plane=4096), dict(n_stack=1, plane=16), dict(D=65)], ids=str)
def test_identities_with_the_one_step_samplers(shape):
    ring = K.history_ring(dev=DEV, **shape)
    pairs = ring.stored_pairs()
    for pool in (False, True):
        one = one_step_gpu(ring, pairs, pool)
        got = run_nstep(ring, 1, 0.99, pool, pairs)
        for k in U.FIELDS:                                  # n_steps = 1: every shared output, bit for bit
            assert np.array_equal(bits(got[k]), bits(one[k])), (k, pool)
        assert (got["steps"] == 1).all() and (got["discounts"] == np.float32(0.99)).all()
        for n_steps in (2, 5, 64):                          # any n: next_obs and done are the one-step sampler's at (L, e)
            got = run_nstep(ring, n_steps, 0.99, pool, pairs)
            last = np.stack([(pairs[:, 0] + got["steps"].astype(np.int32) - 1) % ring.C, pairs[:, 1]], 1).astype(np.int32)
            at_last = one_step_gpu(ring, last, pool)
            for k in ("next_observations", "dones"):
                assert np.array_equal(bits(got[k]), bits(at_last[k])), (k, n_steps, pool)
            for k in ("observations", "actions", "indices"):
                assert np.array_equal(bits(got[k]), bits(one[k])), (k, n_steps, pool)


# ---- 5. through the env and the buffer ------------------------------------------------------------------------------------------------------
B = 4
MODES = [("birdview", 3, {}), ("birdview", 1, {}), ("vector", 1, dict(vector_obs=VectorObs(k_neighbours=2, n_rays=4)))]


@pytest.fixture(scope="module")
def world():
    from torchdriveenv_amd.synth import synthetic_world

    return synthetic_world(n_scn=4, A=4)


def ref_of(buf):
    """the restatement over the buffer's own tensors"""
    kw = dict(n_stack=buf.n_stack, plane=buf.plane, D=buf.D)
    ref = T.TerminalRing(buf.C, buf.B, buf.M, **kw) if buf.tstruct is not None else R.Ring(buf.C, buf.B, **kw)
    for k in buf._tensors:
        setattr(ref, k, getattr(buf, k).cpu().numpy())
    ref.first, ref.w, ref.count = buf.first, buf.w, buf.count
    return ref


def same_batch(got, want):
    for k in FIELDS:
        g = getattr(got, k).cpu().numpy()
        assert np.array_equal(bits(g.reshape(want[k].shape)), bits(want[k])), k


@pytest.mark.parametrize("terminal_obs", (False, True))
@pytest.mark.parametrize("obs_mode,frame_stack,kw", MODES, ids=["birdview3", "birdview1", "vector"])
def test_sample_nstep_over_an_env(world, obs_mode, frame_stack, kw, terminal_obs):
    cfg = EnvConfig(seed=7, distance_cutoff=0.25, max_environment_steps=5, frame_stack=frame_stack,
                    simulator=SimulatorConfig(renderer=RendererConfig(res=64)))
    env = BatchedWaypointEnv(cfg, world, num_envs=B, device=DEV, obs_mode=obs_mode, frame_stack=frame_stack, terminal_obs=terminal_obs, **kw)
    buf = env.replay_buffer(16, seed=3)
    rng = np.random.default_rng(1)
    env.reset()
    buf.begin()
    for _ in range(12):
        a = torch.from_numpy(np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)).to(DEV)
        env.step(a)
        buf.push(a)
    ref = ref_of(buf)
    assert ((ref.done & 3) != 0).sum() >= 2 * B             # every env ran out of steps twice: episodes end inside the look-ahead
    pairs = ref.valid_pairs()
    assert np.array_equal(buf.valid_pairs().cpu().numpy(), pairs)
    for n_steps, gamma in ((1, 0.99), (3, 0.99), (5, 0.5), (64, 1.0)):
        draws = buf.draws
        got = buf.sample_nstep(64, n_steps, gamma)
        assert buf.draws == draws + 1
        same_batch(got, N.gather(ref, ref.draw(buf.seed, draws, 64), n_steps, gamma))
        got = buf.sample_nstep(None, n_steps, gamma, idx=torch.from_numpy(pairs))
        assert buf.draws == draws + 1                       # given pairs draw nothing
        same_batch(got, N.gather(ref, pairs, n_steps, gamma))
        m = got.steps.cpu().numpy()
        assert m.min() >= 1 and (n_steps == 1 or m.max() > 1)
        assert torch.equal(got.bootstrap, torch.from_numpy(T.bootstrap_mask(got.dones.cpu().numpy())).to(DEV))
    assert terminal_obs == bool((got.dones & U.HAS).any())
    # sample() and sample_nstep(n, 1) from equal counters agree
    draws = buf.draws
    one = buf.sample(32)
    buf.draws = draws
    nst = buf.sample_nstep(32, 1)
    assert buf.draws == draws + 1
    for k in one._fields:
        a, b = getattr(one, k), getattr(nst, k)
        assert a.data_ptr() != b.data_ptr() and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)), k
    assert (nst.steps == 1).all() and (nst.discounts == np.float32(0.99)).all()
    assert buf.sample_nstep(32, 2).observations.data_ptr() == nst.observations.data_ptr()      # kept per n

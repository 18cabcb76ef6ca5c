"""The sequence sample on the GPU (include/tde_sequence.h; ReplayBuffer.sample_sequence).  Nothing here has a tolerance: every output
byte is held to the numpy restatement (tests/sequence_ref.py) - through the C-ABI on rings filled by hand (tests/ring_util.HandRing) with
the histories of tests/sequence_cases.py, whose reasons tests/test_sequence_cpu.py vouches for, into outputs pre-filled with canary bytes
and with canaries around them - to the existing samplers on the same ring where the contract says they agree, and to what a real env
returned."""
import numpy as np
import pytest
import torch

from tests import priority_ref as P
from tests import replay_ref as R
from tests import ring_util as U
from tests import sequence_cases as K
from tests import sequence_ref as S
from tests.ring_util import CUT, HAS, bits, guarded, guards_ok
from tests.terminal_ref import bootstrap_mask
from torchdriveenv_amd import ops
from torchdriveenv_amd.config import EnvConfig, Prioritized, RendererConfig, SimulatorConfig, VectorObs
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.replay import priority_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENDED = R.ENDED


def outputs(ring, n, T):
    obs = ((n, T + 1, 3 * ring.n_stack, ring.plane), torch.uint8) if ring.plane else ((n, T + 1, ring.D), torch.float32)
    spec = {"observations": obs, "actions": ((n, T, 2), torch.float32), "rewards": ((n, T), torch.float32), "dones": ((n, T), torch.uint8),
            "lengths": ((n,), torch.int32), "indices": ((n, 2), torch.int32)}
    whole, out = {}, {}
    for k, (shape, dt) in spec.items():
        whole[k], out[k] = guarded(shape, dt, DEV)          # (the middle holds the canary value too: an unwritten byte shows)
    return whole, out


def run_seq(ring, T, pool, pairs=None, n=None, seed=0, draw=0):
    """tde_sequence_sample of the given pairs, or of n drawn ones, into guarded outputs -> numpy arrays (the canaries checked)"""
    n = len(pairs) if pairs is not None else n
    whole, out = outputs(ring, n, T)
    tin = None if pairs is None else torch.from_numpy(np.asarray(pairs, np.int32).reshape(-1, 2)).to(DEV)
    ops.sequence_sample(ring.rp, ring.tm if pool else None, DEV, ring.first, ring.count, n, T, out, tin, seed, draw)
    for k in S.FIELDS:
        assert guards_ok(whole[k], out[k]), k
    return {k: out[k].cpu().numpy() for k in S.FIELDS}


def check_seq(ring, T, pool, pairs=None, n=None, seed=0, draw=0):
    got = run_seq(ring, T, pool, pairs, n, seed, draw)
    idx = S.draw(ring.ref, seed, draw, n, T) if pairs is None else pairs
    want = S.gather(ring.ref, idx, T, terminal=pool)
    for k in S.FIELDS:
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), (k, T, pool)
    return got


def with_invalid(pairs):
    """the valid pairs with the invalid ones spread among them"""
    out, bad = [tuple(p) for p in pairs], list(K.INVALID)
    for j, p in enumerate(bad):
        out.insert((j * 7) % (len(out) + 1), p)
    return np.array(out, np.int32)


# ---- 1. the history of every reason, at every shape --------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,plane", K.PLANES)
def test_planes_against_the_restatement(ns, plane):
    ring = K.history_ring(ns, plane=plane, dev=DEV)
    assert ring.check_state() == (6, 5, 11)
    pairs = with_invalid(ring.stored_pairs())
    for pool in (False, True):
        for T in K.T_STEPS:
            got = check_seq(ring, T, pool, pairs)
            assert got["lengths"].min() == 0 and got["lengths"].max() == min(T, ring.count)
            if ring.count - (ns - 1) > 0:
                got = check_seq(ring, T, pool, n=33, seed=U.DRAW_SEED, draw=T)
                assert got["lengths"].min() >= 1
    ring.check_state()                                      # the call reads the ring


@pytest.mark.parametrize("D", K.ROWS)
def test_rows_against_the_restatement(D):
    ring = K.history_ring(D=D, dev=DEV)
    assert ring.check_state() == (6, 5, 11)
    pairs = with_invalid(ring.stored_pairs())
    for pool in (False, True):
        for T in K.T_STEPS:
            check_seq(ring, T, pool, pairs)
            check_seq(ring, T, pool, n=33, seed=U.DRAW_SEED, draw=2**32 + T)
        for n in (1, 3, 4, 5):                              # four windows per workgroup of the scalars: a last workgroup that is not full
            check_seq(ring, 5, pool, pairs[7:7 + n])
    ring.check_state()


def test_the_length_search_beyond_one_round():
    ring = K.long_ring(dev=DEV)
    assert ring.check_state() == (0, 280, 280)
    pairs = K.long_pairs()
    for pool in (False, True):
        for T in K.LONG_T:
            got = check_seq(ring, T, pool, pairs)
            for start, m in K.LONG_LENGTHS.items():
                i = int(np.flatnonzero((pairs == (start, 0)).all(1))[0])
                assert got["lengths"][i] == min(m, T)
        check_seq(ring, 256, pool, n=65, seed=1, draw=2)


@pytest.mark.parametrize("shape", [dict(n_stack=8, plane=16), dict(n_stack=3, plane=16), dict(D=5)], ids=str)
def test_a_saturated_age_along_a_window(shape):
    ring = K.age_ring(dev=DEV, **shape)
    ring.check_state()
    assert (ring.t["age"][:, 0] == 255).all()
    pairs = ring.stored_pairs()
    for pool in (False, True):
        for T in (5, 17):
            check_seq(ring, T, pool, pairs)


@pytest.mark.parametrize("name", list(U.DRAW_CASES))
def test_the_draw_of_one_step_is_the_one_step_samplers(name):
    ring = U.draw_ring(name, DEV)
    lists = []
    for draw in U.DRAWS:
        one, _ = ring.check_sample(n=U.DRAW_N, seed=U.DRAW_SEED, draw=draw)
        for pool in (False, True):
            got = check_seq(ring, 1, pool, n=U.DRAW_N, seed=U.DRAW_SEED, draw=draw)
            assert np.array_equal(got["indices"], one["indices"])
        for T in (2, 3, 256):                               # a longer window draws from a shorter span, or from its first offset alone
            check_seq(ring, T, True, n=U.DRAW_N, seed=U.DRAW_SEED, draw=draw)
        lists.append(got["indices"].tobytes())
    assert len(set(lists)) == len(U.DRAWS)


# ---- 2. against the existing kernels on the same ring -----------------------------------------------------------------------------------
def one_step_gpu(ring, pairs, pool):
    n = len(pairs)
    obs = ((n, 3 * ring.n_stack, ring.plane), torch.uint8) if ring.plane else ((n, ring.D), torch.float32)
    out = {"observations": torch.empty(*obs[0], dtype=obs[1], device=DEV), "next_observations": torch.empty(*obs[0], dtype=obs[1], device=DEV),
           "actions": torch.empty((n, 2), device=DEV), "rewards": torch.empty(n, device=DEV),
           "dones": torch.empty(n, dtype=torch.uint8, device=DEV), "indices": torch.empty((n, 2), dtype=torch.int32, device=DEV)}
    tin = torch.from_numpy(np.asarray(pairs, np.int32).reshape(-1, 2)).to(DEV)
    if pool:
        ops.terminal_sample(ring.rp, ring.tm, DEV, ring.first, ring.count, n, out, tin)
    else:
        ops.replay_sample(ring.rp, DEV, ring.first, ring.count, n, out, tin)
    return {k: v.cpu().numpy() for k, v in out.items()}


def nstep_steps_gpu(ring, pairs, pool, T):
    n = len(pairs)
    obs = ((n, 3 * ring.n_stack, ring.plane), torch.uint8) if ring.plane else ((n, ring.D), torch.float32)
    out = {"observations": torch.empty(*obs[0], dtype=obs[1], device=DEV), "next_observations": torch.empty(*obs[0], dtype=obs[1], device=DEV),
           "actions": torch.empty((n, 2), device=DEV), "rewards": torch.empty(n, device=DEV),
           "dones": torch.empty(n, dtype=torch.uint8, device=DEV), "indices": torch.empty((n, 2), dtype=torch.int32, device=DEV),
           "discounts": torch.empty(n, device=DEV), "steps": torch.empty(n, dtype=torch.uint8, device=DEV)}
    tin = torch.from_numpy(np.asarray(pairs, np.int32).reshape(-1, 2)).to(DEV)
    ops.nstep_sample(ring.rp, ring.tm if pool else None, DEV, ring.first, ring.count, n, T, 0.99, out, tin)
    return out["steps"].cpu().numpy()


@pytest.mark.parametrize("shape", [dict(n_stack=3, plane=2304), dict(n_stack=8, plane=4096), dict(n_stack=1, plane=16), dict(D=65)], ids=str)
def test_identities_with_the_existing_samplers(shape):
    ring = K.history_ring(dev=DEV, **shape)
    pairs = ring.stored_pairs()
    for pool in (False, True):
        one = one_step_gpu(ring, pairs, pool)
        got = run_seq(ring, 1, pool, pairs)                 # T = 1: the one-step sampler's outputs, bit for bit
        for k, mine in (("observations", got["observations"][:, 0]), ("next_observations", got["observations"][:, 1]),
                        ("actions", got["actions"][:, 0]), ("rewards", got["rewards"][:, 0]), ("dones", got["dones"][:, 0]),
                        ("indices", got["indices"])):
            assert np.array_equal(bits(mine), bits(one[k])), (k, pool)
        assert (got["lengths"] == 1).all()
        for T in (2, 5, 11, 17):
            got = run_seq(ring, T, pool, pairs)
            m = got["lengths"]
            assert np.array_equal(m, nstep_steps_gpu(ring, pairs, pool, T))
            for k in range(T + 1):
                step = np.stack([(pairs[:, 0] + k) % ring.C, pairs[:, 1]], 1).astype(np.int32)
                at = one_step_gpu(ring, step, pool)
                live, last = k < m, k == m - 1
                assert np.array_equal(bits(got["observations"][live, k]), bits(at["observations"][live])), (k, T, pool)
                if k + 1 <= T:
                    assert np.array_equal(bits(got["observations"][last, k + 1]), bits(at["next_observations"][last])), (k, T, pool)
                if k < T:
                    for f, g in (("actions", "actions"), ("rewards", "rewards"), ("dones", "dones")):
                        assert np.array_equal(bits(got[f][live, k]), bits(at[g][live])), (f, k, T, pool)
                        assert not bits(got[f][~live, k]).any()
                assert not bits(got["observations"][k > m, k]).any()


# ---- 3. through the env and the buffer ------------------------------------------------------------------------------------------------------
B = 8
EPISODE = 7                                                 # max_environment_steps: no window is longer
MODES =[("birdview", 3, {}), ("birdview", 1, {}), ("vector", 1, dict(vector_obs=VectorObs(k_neighbours=2, n_rays=4)))]
MODE_IDS = ["birdview3", "birdview1", "vector"]


@pytest.fixture(scope="module")
def world():
    from torchdriveenv_amd.synth import synthetic_world

    return synthetic_world(n_scn=4, A=4)


def make_env(world, obs_mode, frame_stack, terminal_obs, **kw):
    cfg = EnvConfig(seed=7, distance_cutoff=0.25, max_environment_steps=EPISODE, frame_stack=frame_stack,
                    simulator=SimulatorConfig(renderer=RendererConfig(res=64)))
    return BatchedWaypointEnv(cfg, world, num_envs=B, device=DEV, obs_mode=obs_mode, frame_stack=frame_stack, terminal_obs=terminal_obs, **kw)


def drive(env, buf, steps, reset_at, mask, seed=1):
    """`steps` steps with a reset(mask=) / begin(mask=) after step `reset_at`; returns the observations the env returned, obs[t] being
    the one step t was taken from (the masked envs' after the reset)"""
    rng = np.random.default_rng(seed)
    obs = [env.reset().cpu().numpy().copy()]
    buf.begin()
    for t in range(steps):
        a = torch.from_numpy(np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)).to(DEV)
        o, *_ = env.step(a)
        buf.push(a)
        obs.append(o.cpu().numpy().copy())
        if t == reset_at:
            dm = torch.from_numpy(mask).to(DEV)
            obs[-1] = env.reset(mask=dm).cpu().numpy().copy()
            buf.begin(mask=dm)
    return np.stack(obs)


def same_bytes(a, b):
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


@pytest.mark.parametrize("terminal_obs", (False, True))
@pytest.mark.parametrize("obs_mode,frame_stack,kw", MODES, ids=MODE_IDS)
def test_sample_sequence_over_an_env(world, obs_mode, frame_stack, kw, terminal_obs):
    env = make_env(world, obs_mode, frame_stack, terminal_obs, **kw)
    buf = env.replay_buffer(12, seed=3)
    steps = 20
    mask = np.array([0, 1, 0, 0, 1, 0, 0, 0], np.uint8)
    log = drive(env, buf, steps, 14, mask)
    assert buf.count == 11 and ((buf.done & 3) != 0).sum() >= B and ((buf.done & CUT) != 0).sum() == 2
    before = buf.state_dict()
    pairs = buf.valid_pairs()
    slot, e = pairs[:, 0].cpu().numpy().astype(np.int64), pairs[:, 1].cpu().numpy().astype(np.int64)
    t0 = steps - 1 - ((buf.w - 1 - slot) % buf.C)           # the step each pair is
    for T in (1, 3, 11, 17):
        draws = buf.draws
        got = buf.sample_sequence(None, T, idx=pairs)
        assert buf.draws == draws                           # given pairs draw nothing
        m = got.lengths.cpu().numpy()
        obs = got.observations.cpu().numpy()
        assert m.min() >= 1 and m.max() == min(T, EPISODE) and same_bytes(got.indices, pairs)      # (some env runs its episode out)
        assert np.array_equal(m, buf.sample_nstep(None, T, idx=pairs).steps.cpu().numpy())
        msk = got.mask.cpu().numpy()
        assert msk.shape == (len(pairs), T) and np.array_equal(msk.sum(1), m)
        for k in range(T + 1):
            live = k < m
            want = log[np.minimum(t0 + k, steps), e]        # what the env returned for that step
            assert np.array_equal(bits(obs[live, k].reshape(want[live].shape)), bits(want[live])), (k, T)
            assert not bits(obs[k > m, k]).any()
            if k < T:
                assert not bits(got.actions.cpu().numpy()[~live, k]).any() and not got.dones.cpu().numpy()[~live, k].any()
                assert not bits(got.rewards.cpu().numpy()[~live, k]).any()
        # the entry behind the last step is next_observations of that step; bootstrap and terminal are ReplaySamples' of it
        last = torch.stack([(pairs[:, 0] + got.lengths - 1) % buf.C, pairs[:, 1]], 1)
        at_last = buf.sample(None, idx=last, check=False)
        rows = torch.arange(len(pairs), device=DEV)
        assert same_bytes(got.observations[rows, got.lengths.long()], at_last.next_observations)
        assert same_bytes(got.dones[rows, got.lengths.long() - 1], at_last.dones)
        assert torch.equal(got.bootstrap, at_last.bootstrap) and torch.equal(got.terminal, at_last.terminal)
        assert np.array_equal(got.bootstrap.cpu().numpy(), bootstrap_mask(at_last.dones.cpu().numpy()))
        live_next = ~at_last.terminal.cpu().numpy()         # where the window stopped without an ending the next entry is the env's too
        want = log[np.minimum(t0 + m, steps), e]
        assert np.array_equal(bits(obs[np.arange(len(m)), m][live_next].reshape(want[live_next].shape)), bits(want[live_next]))
        assert got.priorities is None and got.weights is None
    assert terminal_obs == bool((got.dones & HAS).any())
    # a drawn batch: the restatement's starts, the counter advances by one, windows fit
    draws = buf.draws
    got = buf.sample_sequence(64, 5)
    assert buf.draws == draws + 1
    ref = R.Ring(buf.C, buf.B, n_stack=buf.n_stack, plane=buf.plane, D=buf.D)
    ref.first, ref.w, ref.count = buf.first, buf.w, buf.count
    assert np.array_equal(got.indices.cpu().numpy(), S.draw(ref, buf.seed, draws, 64, 5))
    assert same_bytes(got.observations, buf.sample_sequence(None, 5, idx=got.indices, check=False).observations)
    # sample() and sample_sequence(n, 1) from equal counters agree bit for bit
    draws = buf.draws
    one = buf.sample(32)
    buf.draws = draws
    seq = buf.sample_sequence(32, 1)
    assert buf.draws == draws + 1
    for a, b in ((one.observations, seq.observations[:, 0]), (one.next_observations, seq.observations[:, 1]), (one.actions, seq.actions[:, 0]),
                 (one.rewards, seq.rewards[:, 0]), (one.dones, seq.dones[:, 0]), (one.indices, seq.indices)):
        assert same_bytes(a, b)
    assert (seq.lengths == 1).all()
    # side effects: the state is as it was apart from the counter; outputs are kept per (n, length)
    after = buf.state_dict()
    assert sorted(after) == sorted(before) and after["draws"] == before["draws"] + 2
    for k in before:
        if k != "draws":
            assert same_bytes(after[k], before[k]) if torch.is_tensor(before[k]) else after[k] == before[k], k
    a, b, c = buf.sample_sequence(32, 2), buf.sample_sequence(32, 3), buf.sample_sequence(16, 2)
    for f in ("observations", "actions", "rewards", "dones", "lengths", "indices"):
        ptrs = {getattr(x, f).data_ptr() for x in (a, b, c, seq)}
        assert len(ptrs) == 4, f
    assert buf.sample_sequence(32, 2).observations.data_ptr() == a.observations.data_ptr()
    with pytest.raises(ValueError, match="needs a buffer built with prioritized=Prioritized"):
        buf.sample_sequence(4, 3, prioritized=True)


# ---- 4. prioritized starts -----------------------------------------------------------------------------------------------------------------
def statement_of(buf):
    """the Python statement of the priorities over the buffer's own tensors"""
    ring = R.Ring(buf.C, buf.B, n_stack=buf.n_stack, plane=buf.plane, D=buf.D)
    for k in ("frames", "action", "reward", "done", "age"):
        setattr(ring, k, getattr(buf, k).cpu().numpy())
    ring.first, ring.w, ring.count = buf.first, buf.w, buf.count
    pr = P.Priorities(ring)
    pr.leaf, pr.qmax = buf.leaf.cpu().numpy().view(np.uint32).copy(), int(buf.qmax[0])
    return pr


@pytest.mark.parametrize("terminal_obs", (False, True))
def test_prioritized_starts(world, terminal_obs):
    env = make_env(world, "birdview", 3, terminal_obs)
    buf, twin = env.replay_buffer(12, seed=3, prioritized=Prioritized()), env.replay_buffer(12, seed=3, prioritized=Prioritized())
    drive(env, buf, 16, 9, np.array([0, 0, 1, 0, 0, 0, 0, 1], np.uint8))
    every = buf.valid_pairs()
    buf.update_priorities(every, torch.linspace(0.1, 4.0, len(every), device=DEV))
    twin.load_state_dict(buf.state_dict())
    for n, T, beta in ((64, 5, None), (7, 17, 1.0), (64, 1, 0.0)):
        draws = buf.draws
        got = buf.sample_sequence(n, T, prioritized=True, beta=beta)
        assert buf.draws == draws + 1 and twin.draws == draws
        pick = twin.sample_prioritized(n)                   # the same pick from a buffer in the same state
        assert same_bytes(got.indices, pick.indices) and same_bytes(got.priorities, pick.priorities)
        idx, q, _ = statement_of(buf).draw(buf.seed, draws, n)
        assert np.array_equal(got.indices.cpu().numpy(), idx) and np.array_equal(got.priorities.cpu().numpy().view(np.uint32), q)
        b = buf.prioritized.beta if beta is None else beta
        assert same_bytes(got.weights, priority_weights(got.priorities, b))
        assert np.allclose(got.weights.cpu().numpy(), P.weights(q, b), rtol=1e-6, atol=0)
        assert got.lengths.min() >= 1
        kept = {f: getattr(got, f).clone() for f in S.FIELDS}                   # (the next call of the same size reuses the tensors)
        want = buf.sample_sequence(None, T, idx=kept["indices"])
        for f in S.FIELDS:
            assert same_bytes(kept[f], getattr(want, f)), f
    # a window's priority goes back through update_priorities: the next pick is the statement's after the same update
    got = buf.sample_sequence(64, 5, prioritized=True)
    td = torch.rand((64, 5), device=DEV) * got.mask
    seq_priority = 0.9 * td.amax(1) + 0.1 * td.sum(1) / got.lengths.clamp(min=1)
    st = statement_of(buf)
    buf.update_priorities(got.indices, seq_priority)
    p = ((seq_priority.abs() + float(buf.prioritized.eps)) ** float(buf.prioritized.alpha)).cpu().numpy()
    st.update(got.indices.cpu().numpy(), p)
    assert np.array_equal(buf.leaf.cpu().numpy().view(np.uint32), st.leaf) and int(buf.sums[0]) == st.total
    draws = buf.draws
    nxt = buf.sample_sequence(64, 5, prioritized=True)
    idx, q, _ = st.draw(buf.seed, draws, 64)
    assert np.array_equal(nxt.indices.cpu().numpy(), idx) and np.array_equal(nxt.priorities.cpu().numpy().view(np.uint32), q)

"""Prioritized replay on the GPU (include/tde_priority.h; ReplayBuffer.sample_prioritized / update_priorities).  Nothing here has a
tolerance: the picked pairs, their priorities, every leaf, sums[0] and qmax are held bit for bit to the Python statement
(tests/priority_ref.py), which picks by a prefix sum over the flat leaves and knows no tree - through the C-ABI on rings filled by hand
(tests/priority_cases.HandPriorities over tests/ring_util.HandRing), with canaries around every output and around leaf, sums and qmax,
on the case table tests/test_priority_cpu.py vouches for - and through the env and the buffer."""
import numpy as np
import pytest
import torch

from tests import priority_cases as K
from tests import priority_ref as P
from tests import replay_ref as R
from tests import ring_util as U
from torchdriveenv_amd.config import EnvConfig, Prioritized, RendererConfig, SimulatorConfig, VectorObs
from torchdriveenv_amd.env import BatchedWaypointEnv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- 1. the draw, at every shape ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_stack", (1, 3))
@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_draws_against_the_statement(shape, n_stack):
    hp = K.filled(shape, n_stack, DEV)                      # (every push and update checks leaf, sums[0], qmax and the canaries)
    hp.ring.check_state()
    for kind in K.KINDS:
        pairs = hp.set_all(K.priorities_of(kind, hp))
        for n, seed, draw in K.draw_settings(kind, len(pairs)):
            idx, q, _ = hp.draw(n, seed, draw)
            assert (q > 0).all()
    hp.ring.check_state()                                   # no call wrote the ring


def test_nothing_drawable_picks_nothing():
    ring = U.HandRing(4, 5, 3, plane=16, dev=DEV, seed=2)
    hp = K.HandPriorities(ring)
    ring.begin(ring.rows())
    hp.reset()
    assert hp.ref.total == 0 and ring.count == 0
    for n in (1, 7, 256):
        idx, q, _ = hp.draw(n, K.SEED, n)
        assert (idx == -1).all() and not q.any()
    hp.step()                                               # one drawable slot: every sample picks from it
    idx, q, _ = hp.draw(7, K.SEED, 0)
    assert (idx[:, 0] == 0).all() and (q == P.ONE).all()


# ---- 2. updates ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ("partial_block", "three_levels"))
def test_updates(shape):
    hp = K.filled(shape, 3, DEV)
    g = hp.ring.ref
    ok = P.valid_mask(g)
    good = g.valid_pairs()
    stored_not_whole = [(s, e) for s in range(g.C) for e in range(g.B) if (s - g.first) % g.C < g.count and not ok[s, e]]
    assert stored_not_whole
    # quantisation edges, one pair each
    edges = np.array([p for p, _ in K.QUANT_EDGES], np.float32)
    assert hp.update(good[:len(edges)], edges) == len(edges)
    assert [int(hp.ref.leaf[s, e]) for s, e in good[:len(edges)]] == [w for _, w in K.QUANT_EDGES] and hp.ref.qmax == P.QMAX
    # duplicates: the largest wins, in any order
    a, b = good[20], good[21]
    hp.update([a, b, a, a, b], np.array([2.0, 7.0, 5.0, 3.0, 1.0], np.float32))
    assert hp.ref.leaf[a[0], a[1]] == 5 * P.ONE and hp.ref.leaf[b[0], b[1]] == 7 * P.ONE
    hp.update([a, a], np.array([0.25, 0.125], np.float32))  # and it replaces what was there: not max with the old leaf
    assert hp.ref.leaf[a[0], a[1]] == P.ONE // 4
    # ignored pairs between valid ones: out of range, the open slot, stored pairs whose stack the ring has overwritten
    bad = [(-1, 0), (g.C, 0), (0, -1), (0, g.B), (U.INT32_MIN, 0), (0, U.INT32_MAX), (g.w, 2), stored_not_whole[0], stored_not_whole[-1]]
    mixed = [p for pair in zip(bad, good[30:30 + len(bad)].tolist()) for p in pair]
    before = hp.ref.leaf.copy()
    assert hp.update(mixed, np.full(len(mixed), 9.0, np.float32)) == len(bad)
    assert all(hp.ref.leaf[s, e] == 0 for s, e in bad[6:]) and (hp.ref.leaf != before).sum() == len(bad)
    assert shape != "three_levels" or len(good) >= 257
    for n in sorted({1, 4, min(257, len(good))}):           # 256 entries per workgroup: a last one that is not full
        hp.update(good[:n], np.linspace(0.5, 3.0, n).astype(np.float32))
    hp.draw(256, K.SEED, 9)


def test_qmax_is_carried_into_the_next_push():
    hp = K.filled("one_level", 1, DEV)
    pairs = hp.ring.ref.valid_pairs()
    hp.update(pairs[:1], np.array([3.5], np.float32))
    assert hp.ref.qmax == 7 * P.ONE // 2
    hp.step()
    g = hp.ring.ref
    assert (hp.ref.leaf[(g.w - 1) % g.C] == 7 * P.ONE // 2).all() and not hp.ref.leaf[g.w].any()
    hp.update(pairs[1:2], np.array([1.0], np.float32))      # a smaller priority leaves qmax
    hp.step()
    assert (hp.ref.leaf[(hp.ring.w - 1) % g.C] == 7 * P.ONE // 2).all()
    hp.reset()
    assert hp.ref.qmax == P.ONE and hp.ref.total == 0


# ---- 3. pushes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_stack", (1, 3))
def test_pushes_through_two_wraps_and_a_masked_begin(n_stack):
    ring = U.HandRing(4, 5, n_stack, plane=16, dev=DEV, seed=5)
    hp = K.HandPriorities(ring)
    ring.begin(ring.rows())
    hp.reset()
    for t in range(2 * 4 + 3):                              # (the invariant, the leaves, sums[0], qmax: checked after every call)
        if t == 5:
            hp.begin(mask=[1, 0, 1, 0, 0])
        hp.step((ring.rng.uniform(size=5) < 0.3) * ring.rng.integers(1, 4, 5))
        hp.draw(7, K.SEED, t)
    ring.check_state()


def test_a_saturated_age():
    ring = U.HandRing(5, 2, 3, plane=16, dev=DEV, seed=6)
    hp = K.HandPriorities(ring)
    ring.begin(ring.rows())
    hp.reset()
    for t in range(260):
        hp.step([0, 1] if t % 7 == 6 else None)             # env 0 never ends: its age saturates; env 1 is young again and again
    assert (ring.ref.age[:, 0] == 255).all() and ring.ref.age[:, 1].max() < 7
    assert hp.ref.leaf[:, 0].astype(bool).sum() == 2        # of env 0's four stored steps the two oldest have lost their stacks
    hp.draw(7, K.SEED, 0)


# ---- 4. through the env and the buffer --------------------------------------------------------------------------------------------------------
B = 4
MODES = [("birdview", 3, {}), ("birdview", 1, {}), ("vector", 1, dict(vector_obs=VectorObs(k_neighbours=2, n_rays=4)))]


@pytest.fixture(scope="module")
def world():
    from torchdriveenv_amd.synth import synthetic_world

    return synthetic_world(n_scn=4, A=4)


def statement_of(buf):
    """the Python statement over the buffer's own tensors"""
    ring = R.Ring(buf.C, buf.B, n_stack=buf.n_stack, plane=buf.plane, D=buf.D)
    for k in ("frames", "action", "reward", "done", "age"):
        setattr(ring, k, getattr(buf, k).cpu().numpy())
    ring.first, ring.w, ring.count = buf.first, buf.w, buf.count
    pr = P.Priorities(ring)
    pr.leaf, pr.qmax = buf.leaf.cpu().numpy().view(np.uint32).copy(), int(buf.qmax[0])
    return pr


def same_bytes(a, b):
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


@pytest.mark.parametrize("terminal_obs", (False, True))
@pytest.mark.parametrize("obs_mode,frame_stack,kw", MODES, ids=["birdview3", "birdview1", "vector"])
def test_sample_prioritized_over_an_env(world, obs_mode, frame_stack, kw, terminal_obs):
    cfg = EnvConfig(seed=7, distance_cutoff=0.25, max_environment_steps=5, frame_stack=frame_stack,
                    simulator=SimulatorConfig(renderer=RendererConfig(res=64)))
    env = BatchedWaypointEnv(cfg, world, num_envs=B, device=DEV, obs_mode=obs_mode, frame_stack=frame_stack, terminal_obs=terminal_obs, **kw)
    buf = env.replay_buffer(8, seed=3, prioritized=Prioritized())
    plain = env.replay_buffer(8, seed=3)
    assert plain.pstruct is None and plain.leaf is None and "leaf" not in plain.state_dict()
    rng = np.random.default_rng(1)
    env.reset()
    buf.begin()
    for t in range(12):                                     # the ring of eight slots wraps
        a = torch.from_numpy(np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)).to(DEV)
        env.step(a)
        buf.push(a)
        if t == 6:
            buf.begin()                                     # a repeated begin() changes no priority
        st = statement_of(buf)
        assert np.array_equal(st.leaf != 0, P.valid_mask(st.ring)) and int(buf.sums[0]) == st.total
        assert (st.leaf[st.leaf != 0] == P.ONE).all()
    pairs = {tuple(x) for x in buf.valid_pairs().cpu().tolist()}
    assert buf.count == 7 and len(pairs) == (st.leaf != 0).sum()
    # the batch is sample_nstep's of the picked pairs; the picks are the statement's
    for n, k, gamma in ((64, 1, 0.99), (64, 3, 0.99), (7, 5, 0.5)):
        draws = buf.draws
        got = buf.sample_prioritized(n, k, gamma)
        assert buf.draws == draws + 1
        idx, q, _ = st.draw(buf.seed, draws, n)
        assert np.array_equal(got.indices.cpu().numpy(), idx) and np.array_equal(got.priorities.cpu().numpy().view(np.uint32), q)
        assert {tuple(x) for x in idx.tolist()} <= pairs
        want = buf.sample_nstep(None, k, gamma, idx=got.indices)
        assert buf.draws == draws + 1
        for f in want._fields:
            assert getattr(got, f).data_ptr() != getattr(want, f).data_ptr() and same_bytes(getattr(got, f), getattr(want, f)), f
        assert np.allclose(got.weights.cpu().numpy(), P.weights(q, 0.4), rtol=1e-6, atol=0) and (got.weights == 1).all()
        assert buf.sample_prioritized(n, k, gamma, beta=1.0).observations.data_ptr() == got.observations.data_ptr()     # kept per n
    # sample() and sample_nstep() stay the uniform draws
    draws = buf.draws
    plain.load_state_dict({k: v for k, v in buf.state_dict().items() if k not in ("leaf", "qmax")})
    uni = buf.sample(32)
    assert plain.draws == draws and same_bytes(plain.sample(32).indices, uni.indices)
    # one pair raised to the top, the others lowered: its count over eight draws of 64 is the statement's
    every = buf.valid_pairs()
    top = every[len(every) // 2]
    td = torch.zeros(len(every), device=DEV)
    td[len(every) // 2] = 1e9
    buf.update_priorities(torch.cat([every, top[None]]), torch.cat([td, torch.zeros(1, device=DEV)]))      # named twice: the larger wins
    st = statement_of(buf)
    low = st.leaf[st.leaf != 0].min()
    assert st.leaf[top[0], top[1]] == P.QMAX == st.qmax and low < 100 and (st.leaf == low).sum() == len(every) - 1
    assert int(buf.sums[0]) == st.total
    draws, count, want_count = buf.draws, 0, 0
    for d in range(8):
        got = buf.sample_prioritized(64, 3)
        count += int(((got.indices == top).all(1)).sum())
        want_count += int((st.draw(buf.seed, draws + d, 64)[0] == top.cpu().numpy()).all(1).sum())
        w = got.weights.cpu().numpy()
        assert np.allclose(w, P.weights(got.priorities.cpu().numpy(), 0.4), rtol=1e-6, atol=0)
    assert count == want_count >= 8 * 60
    # the state round-trips the next draw; the sums are rebuilt on load
    sd = buf.state_dict()
    first = buf.sample_prioritized(32, 3)
    keep = {f: getattr(first, f).clone() for f in first._fields}
    other = env.replay_buffer(8, seed=99, prioritized=Prioritized())
    other.load_state_dict(sd)
    assert int(other.sums[0]) == st.total and other.seed == buf.seed
    again = other.sample_prioritized(32, 3)
    for f in first._fields:
        assert same_bytes(keep[f], getattr(again, f)), f
    with pytest.raises(ValueError, match="with priorities, this buffer is without"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="without priorities, this buffer is with "):
        other.load_state_dict(plain.state_dict())
    # an index sampled before the ring overwrote its slot does not resurrect a dead leaf
    stale = torch.tensor([[buf.first, 0]], dtype=torch.int32, device=DEV)
    a = torch.zeros((B, 2), device=DEV)
    env.step(a)
    buf.push(a)
    buf.update_priorities(stale, torch.ones(1, device=DEV))
    st = statement_of(buf)
    assert st.leaf[stale[0, 0], 0] == 0 and np.array_equal(st.leaf != 0, P.valid_mask(st.ring)) and int(buf.sums[0]) == st.total
    assert (st.leaf[(buf.w - 1) % buf.C] == P.QMAX).all()   # the pushed step entered with qmax


# ---- 5. every depth of the tree, leaf counts that fill their blocks, installed leaves ------------------------------------------------------------
@pytest.mark.parametrize("shape,n_stack", [(s, 1) for s in K.DEPTH_SHAPES] + [(s, 3) for s in K.DEPTH_STACKED])
def test_depth_shapes_reset_push_update(shape, n_stack):
    """reset over rubbish (every leaf and EVERY word of sums zero), pushes until the ring wraps, two updates of hundreds of pairs spread
    over the flat range and one more push, a draw of 256 after each (tests/priority_cases.depth_run): leaf, sums[0], qmax and the
    canaries after every call, every pick the statement's"""
    c = K.DEPTH_SHAPES[shape]
    hp, rounds = K.depth_run(shape, n_stack, DEV)
    assert hp.t["sums"].numel() == c["words"] and hp.ring.count == c["C"] - 1
    assert all((q > 0).all() for _, _, q in rounds)
    hp.ring.check_state()                                   # no call wrote the ring


@pytest.mark.parametrize("shape,pattern", K.INSTALLED_CASES)
def test_installed_leaves_are_picked_as_the_statement_picks(shape, pattern):
    """a named pattern of leaves put into the device tree, every draw setting; a second pattern over it without a reset, drawn again;
    a real push and a real update on top, drawn once more (tests/priority_cases.installed_run; tests/test_priority_cpu.py vouches for
    what the patterns and the draws reach)"""
    n = K.DEPTH_SHAPES[shape]["n"]
    hp, recs = K.installed_run(shape, pattern, DEV)
    assert {r["stage"] for r in recs} == {0, 1, 2} and all((r["q"] > 0).all() for r in recs)
    for name, want in (("last_only", n - 1), ("first_only", 0)):       # the one live pair, whatever the position
        for r in recs:
            assert r["stage"] == 2 or r["pattern"] != name or ((r["l"] == want).all() and (r["q"] == 1).all()), (name, r["N"])
    assert pattern not in ("last_only", "first_only") or sum(r["pattern"] == pattern for r in recs) == 4
    hp.ring.check_state()


@pytest.mark.parametrize("shape", ("tail_4", "tail_2"))
def test_nothing_drawable_at_depth(shape):
    hp = K.depth_ring(shape, 1, DEV)
    hp.reset()
    assert hp.ref.total == 0
    for n in (1, 256):
        idx, q, _ = hp.draw(n, K.SEED, n)
        assert (idx == -1).all() and not q.any()


def test_buffer_with_a_two_level_tree(world):
    """the buffer over an env with C * B = 96 leaves: a root over two level-1 nodes, so that pushes, update_priorities and the rebuild
    of load_state_dict have inner nodes besides the total to keep"""
    cfg = EnvConfig(seed=7, distance_cutoff=0.25, max_environment_steps=5, frame_stack=3, simulator=SimulatorConfig(renderer=RendererConfig(res=64)))
    env = BatchedWaypointEnv(cfg, world, num_envs=B, device=DEV, obs_mode="birdview", frame_stack=3)
    buf = env.replay_buffer(24, seed=3, prioritized=Prioritized())
    assert buf.C * buf.B >= 65 and buf.sums.numel() == K.tree_words(buf.C * buf.B) >= 3
    rng = np.random.default_rng(1)
    env.reset()
    buf.begin()
    for t in range(30):                                     # the ring of 24 slots wraps
        if t == 14:
            mask = torch.tensor([1, 0, 0, 1], dtype=torch.uint8, device=DEV)
            env.reset(mask=mask)
            buf.begin(mask=mask)
        a = torch.from_numpy(np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)).to(DEV)
        env.step(a)
        buf.push(a)
        st = statement_of(buf)
        assert np.array_equal(st.leaf != 0, P.valid_mask(st.ring)) and int(buf.sums[0]) == st.total
        assert (st.leaf[st.leaf != 0] == P.ONE).all()
    assert buf.count == 23 and 0 < buf.w < 23
    every = buf.valid_pairs()
    assert len(every) > 64                                  # drawable pairs under both level-1 nodes
    td = torch.from_numpy(np.exp(rng.uniform(np.log(1e-4), np.log(1e4), len(every))).astype(np.float32)).to(DEV)
    buf.update_priorities(every, td)
    st = statement_of(buf)
    assert np.array_equal(st.leaf != 0, P.valid_mask(st.ring)) and int(buf.sums[0]) == st.total
    assert len(np.unique(st.leaf)) > len(every) // 2 and st.qmax == st.leaf.max() > P.ONE
    draws = buf.draws
    got = buf.sample_prioritized(64, 3)
    idx, q, _ = st.draw(buf.seed, draws, 64)
    assert np.array_equal(got.indices.cpu().numpy(), idx) and np.array_equal(got.priorities.cpu().numpy().view(np.uint32), q)
    flat = idx[:, 0].astype(np.int64) * B + idx[:, 1]
    assert (flat < 64).any() and (flat >= 64).any()         # picks under both children of the root
    # the state into a second buffer, whose sums held nothing: load_state_dict rebuilds them, and the next draw is the first buffer's
    sd = buf.state_dict()
    first = buf.sample_prioritized(64, 3)
    keep = {f: getattr(first, f).clone() for f in first._fields}
    other = env.replay_buffer(24, seed=99, prioritized=Prioritized())
    other.sums.fill_(0x0123456789)                          # (nor is what they held before of any account)
    other.load_state_dict(sd)
    assert int(other.sums[0]) == st.total and other.seed == buf.seed
    again = other.sample_prioritized(64, 3)
    idx, q, _ = st.draw(buf.seed, draws + 1, 64)
    assert np.array_equal(again.indices.cpu().numpy(), idx)
    for f in first._fields:
        assert same_bytes(keep[f], getattr(again, f)), f

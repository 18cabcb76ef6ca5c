"""The launches a BatchedWaypointEnv makes, call by call: every method of the env's launch handle (env._h) and the two ring launches the
env and its replay buffer make outside it (ops.replay_pack, ops.terminal_stash) are recorded by name while the env resets, steps six
times (max_environment_steps = 4: every env finishes on the way), is reset under a mask and reset as a whole, with a replay buffer
following where the env can have one.  TABLE holds what the env did BEFORE its observation moved into observe.py, recorded with this
file's own record() on that commit; both bindings must reproduce it.  What it pins down, among others: a state-mode step is one `step`
and nothing else, and the colour-to-plane pack of a terminal_obs step comes before the stash and runs again for the buffer's push."""
import pytest
import torch

from torchdriveenv_amd import ops
from torchdriveenv_amd.config import EnvConfig, RendererConfig, SimulatorConfig, VectorObs
from torchdriveenv_amd.env import BatchedWaypointEnv

pytestmark = pytest.mark.gpu
B, A, DEV, STEPS = 4, 8, "cuda:0", 6
MODES = {"birdview1": ("birdview", 1, {}), "birdview3": ("birdview", 3, {}), "state": ("state", 1, {}),
         "vector": ("vector", 1, dict(vector_obs=VectorObs(k_neighbours=2, n_rays=4)))}
# (auto_reset, terminal_obs): terminal_obs needs auto_reset
OPTIONS = [(True, False), (True, True), (False, False)]

# mode -> (auto_reset, terminal_obs) -> the calls of: reset() + begin() | EACH of the six step() + push() (the recording showed the six
# alike in every configuration) | reset(mask) + begin(mask) | reset() + begin().  There is no buffer without auto_reset.  Both bindings
# recorded the same.
AUTO, TERMINAL, MANUAL = OPTIONS
TABLE = {
    "birdview1": {MANUAL: ("reset render", "step render", "reset_render", "reset render"),
                  AUTO: ("reset render replay_pack", "step render replay_pack", "reset_render replay_pack", "reset render replay_pack"),
                  TERMINAL: ("reset render replay_pack", "step render replay_pack terminal_stash reset_render replay_pack",
                             "reset_render replay_pack", "reset render replay_pack")},
    "birdview3": {MANUAL: ("reset render", "step render", "reset_render", "reset render"),
                  AUTO: ("reset render", "step render", "reset_render", "reset render"),
                  TERMINAL: ("reset render", "step render terminal_stash reset_render", "reset_render", "reset render")},
    "state": {MANUAL: ("reset state_obs", "step", "reset state_obs", "reset state_obs"),
              AUTO: ("reset state_obs", "step", "reset state_obs", "reset state_obs"),
              TERMINAL: ("reset state_obs", "step terminal_stash reset state_obs", "reset state_obs", "reset state_obs")},
    "vector": {MANUAL: ("reset vector_obs", "step vector_obs", "reset vector_obs", "reset vector_obs"),
               AUTO: ("reset vector_obs", "step vector_obs", "reset vector_obs", "reset vector_obs"),
               TERMINAL: ("reset vector_obs", "step vector_obs terminal_stash reset vector_obs", "reset vector_obs", "reset vector_obs")},
}


class Recording:
    """forwards every method of `handle`, noting its name in `log`"""

    def __init__(self, handle, log):
        self._handle, self._log = handle, log

    def __getattr__(self, name):
        fn = getattr(self._handle, name)

        def call(*a, **kw):
            self._log.append(name)
            return fn(*a, **kw)
        return call


def record(world, mode, auto_reset, terminal_obs, binding, patch):
    """the calls of the scenario above as a list of space-joined phases.  patch(obj, name, value) replaces an attribute for the test."""
    obs_mode, frame_stack, kw = MODES[mode]
    cfg = EnvConfig(seed=3, distance_cutoff=0.25, max_environment_steps=4, frame_stack=frame_stack,
                    simulator=SimulatorConfig(renderer=RendererConfig(res=64)))
    env = BatchedWaypointEnv(cfg, world, num_envs=B, device=DEV, obs_mode=obs_mode, frame_stack=frame_stack, auto_reset=auto_reset,
                             terminal_obs=terminal_obs, binding=binding, **kw)
    log = []
    env._h = Recording(env._h, log)
    for name in ("replay_pack", "terminal_stash"):
        def counted(*a, _fn=getattr(ops, name), _name=name, **k):
            log.append(_name)
            return _fn(*a, **k)
        patch(ops, name, counted)
    buf = env.replay_buffer(8) if auto_reset else None
    phases = []

    def phase():
        phases.append(" ".join(log))
        log.clear()

    env.reset()
    if buf is not None:
        buf.begin()
    phase()
    g = torch.Generator().manual_seed(0)
    for _ in range(STEPS):
        a = ((torch.rand(B, 2, generator=g) * 2 - 1) * torch.tensor([1.0, 0.3])).to(DEV)
        env.step(a)
        if buf is not None:
            buf.push(a)
        phase()
    mask = torch.tensor([1, 0, 1, 0], dtype=torch.uint8, device=DEV)
    env.reset(mask=mask)
    if buf is not None:
        buf.begin(mask=mask)
    phase()
    env.reset()
    if buf is not None:
        buf.begin()
    phase()
    torch.cuda.synchronize()
    return phases


@pytest.fixture(scope="module")
def world():
    from torchdriveenv_amd.synth import synthetic_world

    return synthetic_world(n_scn=4, A=A)


@pytest.mark.parametrize("binding", ["ext", "ctypes"])
@pytest.mark.parametrize("auto_reset,terminal_obs", OPTIONS, ids=["auto", "auto-terminal", "manual"])
@pytest.mark.parametrize("mode", list(MODES))
def test_the_env_makes_the_launches_it_made_before_the_observer(world, monkeypatch, mode, auto_reset, terminal_obs, binding):
    got = record(world, mode, auto_reset, terminal_obs, binding, monkeypatch.setattr)
    first, step, masked, full = TABLE[mode][(auto_reset, terminal_obs)]
    assert got == [first] + [step] * STEPS + [masked, full]


def test_the_table_shows_what_it_must():
    """the two properties the table is there to hold, read off its own entries"""
    assert TABLE["state"][AUTO][1] == TABLE["state"][MANUAL][1] == "step"          # a state-mode step() is ONE launch (push() adds none)
    calls = TABLE["birdview1"][TERMINAL][1].split()                               # the pack feeds the stash, and runs again for push()
    assert calls.index("replay_pack") < calls.index("terminal_stash") and calls.count("replay_pack") == 2

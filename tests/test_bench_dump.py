"""bench.py --dump-outputs on the host: what is written, in which dtypes, and the fixed sample of envs that keeps a large output
under 64 MB (the GPU side: tests/test_gpu_edge.py::test_bench_dump_outputs_are_the_last_timed_step)"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _state(B, A, seed):
    g = torch.Generator().manual_seed(seed)
    return SimpleNamespace(B=B, arrays={
        "x": torch.rand(B * A, generator=g), "present": torch.randint(0, 2, (B * A,), dtype=torch.uint8, generator=g),
        "steps": torch.randint(0, 200, (B,), dtype=torch.int32, generator=g), "info": torch.rand(B, 4, dtype=torch.float64, generator=g),
        "action": torch.zeros(B, 2), "act_cache": torch.zeros(B * (A + 1), 2, dtype=torch.int32), "obs": None})


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_writes_every_output_exactly(tmp_path):
    B, A = 64, 8
    st = _state(B, A, 0)
    reward = torch.rand(B)
    bench.dump_outputs(str(tmp_path), st, {"reward": reward})
    got = _load(tmp_path)
    assert sorted(got) == ["info", "present", "reward", "steps", "x"]          # no input, no cache, no sample index
    assert got["x"].dtype == np.float32 and np.array_equal(got["x"], st.arrays["x"].numpy())
    assert got["present"].dtype == np.float32 and np.array_equal(got["present"], st.arrays["present"].numpy())
    assert got["steps"].dtype == np.float64 and np.array_equal(got["steps"], st.arrays["steps"].numpy())
    assert got["info"].dtype == np.float64 and np.array_equal(got["info"], st.arrays["info"].numpy())
    assert np.array_equal(got["reward"], reward.numpy())


def test_dump_outputs_cuts_a_large_output_to_a_fixed_env_sample(tmp_path):
    B, A = 2048, 32
    st = _state(B, A, 1)
    img = torch.randint(0, 256, (B, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))   # 100 MB as float32
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), st, {"birdview": img})
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 10**6
    envs = a["sampled_envs"].astype(np.int64)
    n = len(envs)
    assert 0 < n < B and (np.diff(envs) > 0).all() and envs[-1] < B
    assert a["birdview"].dtype == np.float32 and np.array_equal(a["birdview"], img.numpy()[envs].astype(np.float32))
    assert np.array_equal(a["x"], st.arrays["x"].numpy().reshape(B, A)[envs].reshape(-1))
    assert np.array_equal(a["info"], st.arrays["info"].numpy()[envs])
    assert np.array_equal(a["steps"], st.arrays["steps"].numpy()[envs])

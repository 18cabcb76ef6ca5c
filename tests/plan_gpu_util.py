"""What the GPU tests of the planner, the plan judge and the forecasts share: a host state onto the device, and the kernels through both
bindings held bit for bit against their numpy restatements (tests/planner_ref.py, tests/plan_set_ref.py).  A plain module: test
infrastructure only, nothing in the package imports it."""
import numpy as np
import torch

from tests import plan_set_ref as S
from tests import planner_ref as R
from torchdriveenv_amd import _abi, _ext, ops
from torchdriveenv_amd.state import EnvState

DEV = "cuda:0"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def on_device(world, hs, dev=DEV):
    """(device world, fresh device EnvState holding host state `hs`: an EnvState or a dict of its numpy arrays)"""
    ds = EnvState(len(hs["scn"]), world.A, device=dev)
    ds.load({k: v for k, v in (hs.arrays if hasattr(hs, "arrays") else hs).items() if v is not None})
    return world.to_device(dev), ds


def check_score_plans(cfg, world, hs, pl, seq, knot_len, tail, only=None, forecast=None, what=""):
    """the kernel (both bindings) on the device copy of host state `hs` == the restatement, every output; rows outside `only` keep
    what they held; forecast (float32 [B, T, A, 4]): tde_score_plans_forecast on these rows; returns the restatement's result"""
    B = len(hs["scn"])
    N = seq.shape[1]
    c0, f0 = np.full((B, N), -5.0, np.float32), np.full((B, N), -9, np.int32)
    a0, d0 = np.full((B, 2), -3.0, np.float32), np.full((B, 4), -7, np.int32)
    want = S.score(cfg, world, hs, pl, seq, knot_len, tail, only=only, cost=c0, fail_step=f0, out=a0, diag=d0, forecast=forecast)
    dw, ds = on_device(world, hs)
    m = torch.from_numpy(np.asarray(only, np.uint8)).to(DEV) if only is not None else None
    dseq = torch.from_numpy(np.ascontiguousarray(seq)).to(DEV)
    dfc = torch.from_numpy(np.ascontiguousarray(forecast)).to(DEV) if forecast is not None else None
    for binding in ("ctypes", "ext"):
        cost, fail = torch.from_numpy(c0).to(DEV), torch.from_numpy(f0).to(DEV)
        act, dg = torch.from_numpy(a0).to(DEV), torch.from_numpy(d0).to(DEV)
        if binding == "ctypes":
            ops.score_plans(cfg, dw, ds, pl, dseq, knot_len, tail, m, cost, fail, act, dg, forecast=dfc)
        else:
            _ext.env_handle(cfg, dw, ds).score_plans(dseq, int(knot_len), int(tail), cost, fail, int(pl.horizon), float(pl.v_target),
                                                     float(pl.margin), float(pl.w_progress), float(pl.w_speed), float(pl.w_steer), m, act,
                                                     dg, int(cfg.flags), dfc)
        torch.cuda.synchronize()
        got_f, got_c = fail.cpu().numpy(), cost.cpu().numpy()
        bad = np.argwhere(got_f != want["f"])
        assert len(bad) == 0, (what, binding, "fail_step", len(bad), bad[:6].tolist(), got_f[tuple(bad[0])], want["f"][tuple(bad[0])])
        bad = np.argwhere(bits(got_c) != bits(want["cost"]))
        assert len(bad) == 0, (what, binding, "cost", len(bad), bad[:6].tolist(), got_c[tuple(bad[0])], want["cost"][tuple(bad[0])])
        got_d = dg.cpu().numpy().view(_abi.PLAN_DIAG_DTYPE).reshape(B)
        for n in ("winner", "fail_step", "n_safe"):
            bad = np.flatnonzero(got_d[n] != want["diag"][n])
            assert len(bad) == 0, (what, binding, n, bad[:8].tolist(), got_d[bad[:4]], want["diag"][bad[:4]])
        assert np.array_equal(got_d["cost"].view(np.uint32), want["diag"]["cost"].view(np.uint32)), (what, binding, "diag cost")
        assert np.array_equal(bits(act.cpu().numpy()), bits(want["action"])), (what, binding, "action")
        # without action / diag the same costs are written
        cost2, fail2 = torch.from_numpy(c0).to(DEV), torch.from_numpy(f0).to(DEV)
        if binding == "ctypes":
            ops.score_plans(cfg, dw, ds, pl, dseq, knot_len, tail, m, cost2, fail2, forecast=dfc)
            assert torch.equal(cost2.view(torch.int32), cost.view(torch.int32)) and torch.equal(fail2, fail), (what, "no diag")
    return want


def check_plan_action(cfg, world, hs, pl, only=None, what=""):
    """the kernel (both bindings) on the device copy of host state `hs` == the restatement; returns (actions, diag) of the latter"""
    B = len(hs["scn"])
    fill = only is not None
    act0 = np.full((B, 2), -3.0, np.float32)
    dg0 = np.full((B, 4), -7, np.int32)
    want_a, want_d = R.plan(cfg, world, hs, pl, only=only, out=act0 if fill else None, diag=dg0 if fill else None)
    dw, ds = on_device(world, hs)
    m = torch.from_numpy(np.asarray(only, np.uint8)).to(DEV) if only is not None else None
    for binding in ("ctypes", "ext"):
        out = torch.full((B, 2), -3.0, dtype=torch.float32, device=DEV)
        dg = torch.full((B, 4), -7, dtype=torch.int32, device=DEV)
        if binding == "ctypes":
            ops.plan_action(cfg, dw, ds, pl, out, m, dg)
        else:
            _ext.env_handle(cfg, dw, ds).plan_action(out, [float(v) for v in pl.accelerations], [float(v) for v in pl.steerings],
                                                     int(pl.horizon), float(pl.v_target), float(pl.margin), float(pl.w_progress),
                                                     float(pl.w_speed), float(pl.w_steer), m, dg, int(cfg.flags))
        torch.cuda.synchronize()
        got_a = out.cpu().numpy()
        got_d = dg.cpu().numpy().view(_abi.PLAN_DIAG_DTYPE).reshape(B)
        for n in ("winner", "fail_step", "n_safe"):
            bad = np.flatnonzero(got_d[n] != want_d[n])
            assert len(bad) == 0, (what, binding, n, bad[:8].tolist(), got_d[bad[:4]], want_d[bad[:4]])
        assert np.array_equal(got_d["cost"].view(np.uint32), want_d["cost"].view(np.uint32)), (what, binding, "cost")
        bad = np.argwhere(bits(got_a) != bits(want_a))
        assert len(bad) == 0, (what, binding, bad[:8].tolist(), got_a[bad[0][0]], want_a[bad[0][0]])
    return want_a, want_d

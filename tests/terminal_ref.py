"""numpy statement of the terminal pool beside the replay ring (include/tde_terminal.h): tests/replay_ref.Ring with the pool - the rank
rule of the push (env order, the first M kept, every ref of the slot rewritten) and the sample that returns a pooled frame as the
newest frame of next_obs."""
import numpy as np

from tests.replay_ref import ENDED, PAL, Ring
from torchdriveenv_amd import _abi

HAS = _abi.TERMINAL_HAS


def ranks(done_bits, M):
    """int32 [B]: the pool row of each env of a push - the number of finished envs before it, or -1 when it did not finish or that
    number is M or more"""
    fin = (np.asarray(done_bits, np.uint8) & 3) != 0
    r = np.cumsum(fin) - fin
    return np.where(fin & (r < M), r, -1).astype(np.int32)


class TerminalRing(Ring):
    """a Ring with M pool rows per slot; push() takes the terminal frames [B, plane] / [B, D] as well (only the finished envs' are read)"""

    def __init__(self, C, B, M, n_stack=1, plane=0, D=0):
        super().__init__(C, B, n_stack, plane, D)
        assert 1 <= M <= B
        self.M = M
        self.pool = np.full((C, M, plane), _abi.LAYER_BLANK, np.uint8) if plane else np.zeros((C, M, D), np.float32)
        self.ref = np.full((C, B), -1, np.int32)

    def push(self, action, reward, done_bits, src, term_src):
        w = self.w
        r = ranks(done_bits, self.M)
        self.ref[w] = r
        keep = r >= 0
        self.pool[w, r[keep]] = np.asarray(term_src)[keep]
        super().push(action, reward, done_bits, src)

    def gather(self, idx):
        out = super().gather(idx)
        idx = np.asarray(idx, np.int64).reshape(-1, 2)
        ns = self.n_stack
        for i, (s, e) in enumerate(idx):
            if not (0 <= s < self.C and 0 <= e < self.B) or int(self.offset(s)) >= self.count:
                continue
            r = int(self.ref[s, e])
            if not (self.done[s, e] & 3) or r < 0:
                continue
            assert self.done[s, e] & ENDED and not out["next_observations"][i].any()
            out["dones"][i] |= HAS
            if self.plane:
                nxt = out["next_observations"][i].reshape(ns, 3, self.plane)
                nxt[:ns - 1] = out["observations"][i].reshape(ns, 3, self.plane)[1:]
                nxt[ns - 1] = PAL[self.pool[s, r]].T
            else:
                out["next_observations"][i] = self.pool[s, r]
        return out


def bootstrap_mask(dones):
    """ReplaySamples.bootstrap"""
    d = np.asarray(dones, np.uint8)
    return ((d & ENDED) == 0) | (((d & 3) == 2) & ((d & HAS) != 0))

"""One rollout append of R runs (csrc/store.hip: orl_buffer_append_rollout / orl_buffer_append_rollout_runs) restated in numpy: the
rows of run r at ring rows ``(ptr + i) % cap`` with 0 / 1 terminals, the survivors' next_obs in their original order, their count, and
the float64 reward sum IN THE DEVICE'S ORDER -- 256 rows per block, 64 lanes per wave: per wave the tree ``v[:o] = v[:o] + v[o:2 * o]``
for o = 32 .. 1 on the zero-padded lanes, the block as ``((w0 + w1) + w2) + w3``, then the blocks in order from 0.0.  The verdicts are
the device's float32 comparisons.  test_store_refs_cpu.py pins this file to utils/termination_fns.py, the recorded verdicts and
math.fsum; test_gpu_store.py compares the device with it, bit for bit and sum for sum."""
import numpy as np

TERM_NONE, TERM_HALFCHEETAH, TERM_HOPPER, TERM_WALKER2D, TERM_ANT, TERM_HUMANOID, TERM_PEN = range(7)
_F = np.float32


def term_done(kind, next_obs):
    """bool [n]: the verdict of termination kind ``kind`` on float32 rows; every comparison is false on NaN"""
    x = np.asarray(next_obs, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        if kind == TERM_NONE:
            return np.zeros(len(x), dtype=bool)
        if kind == TERM_HALFCHEETAH:
            return ~((x > _F(-100)) & (x < _F(100))).all(axis=1)
        if kind == TERM_HOPPER:              # the upper bound alone, on columns 1..
            ok = np.isfinite(x).all(axis=1) & (x[:, 1:] < _F(100)).all(axis=1)
            return ~(ok & (x[:, 0] > _F(.7)) & (np.abs(x[:, 1]) < _F(.2)))
        if kind == TERM_WALKER2D:
            inside = ((x > _F(-100)) & (x < _F(100))).all(axis=1)
            return ~(inside & (x[:, 0] > _F(0.8)) & (x[:, 0] < _F(2.0)) & (x[:, 1] > _F(-1.0)) & (x[:, 1] < _F(1.0)))
        if kind == TERM_ANT:
            return ~(np.isfinite(x).all(axis=1) & (x[:, 0] >= _F(0.2)) & (x[:, 0] <= _F(1.0)))
        if kind == TERM_HUMANOID:
            return (x[:, 0] < _F(1.0)) | (x[:, 0] > _F(2.0))
        if kind == TERM_PEN:
            return x[:, 26] < _F(0.075)
    raise ValueError(f"unknown termination kind {kind}")


def ordered_sum(rew):
    """the float64 sum of float32 rewards in the device's order (see the module text); 0.0 for no rows"""
    rew = np.asarray(rew, dtype=np.float32).ravel()
    total = np.float64(0.0)
    for b0 in range(0, len(rew), 256):
        v = np.zeros(256, dtype=np.float64)
        blk = rew[b0:b0 + 256]
        v[:len(blk)] = blk
        v = v.reshape(4, 64)
        o = 32
        while o > 0:
            v[:, :o] = v[:, :o] + v[:, o:2 * o]
            o >>= 1
        w = v[:, 0]
        total = total + (((w[0] + w[1]) + w[2]) + w[3])
    return total


class Ring:
    """a ring of ``cap`` rows as orl_buffer_reserve leaves it: zeros, nothing appended"""

    def __init__(self, cap, od, ad):
        self.cap, self.ptr, self.size = cap, 0, 0
        self.obs, self.nobs = np.zeros((cap, od), np.float32), np.zeros((cap, od), np.float32)
        self.act = np.zeros((cap, ad), np.float32)
        self.rew, self.term = np.zeros((cap, 1), np.float32), np.zeros((cap, 1), np.float32)

    def columns(self):
        """in DeviceBuffer.read_rows' order"""
        return self.obs, self.act, self.nobs, self.rew, self.term


def append_rollout(rings, kind, obs, act, next_obs, rew, n, alive_next_obs):
    """``rings[r]`` receives the first ``n[r]`` rows of obs / next_obs [R, stride, od], act [R, stride, ad], rew [R, stride];
    ``alive_next_obs`` [R, stride, od] is written in place, the survivors of run r at the front of its block and nothing else.
    Returns (n_alive int64 [R], reward sums float64 [R])."""
    R = len(rings)
    n_alive, sums = np.zeros(R, np.int64), np.zeros(R, np.float64)
    for r, g in enumerate(rings):
        k = int(n[r])
        assert 0 <= k <= g.cap
        done = term_done(kind, next_obs[r, :k])
        where = (g.ptr + np.arange(k)) % g.cap
        g.obs[where], g.nobs[where], g.act[where] = obs[r, :k], next_obs[r, :k], act[r, :k]
        g.rew[where, 0], g.term[where, 0] = rew[r, :k], done.astype(np.float32)
        g.ptr, g.size = (g.ptr + k) % g.cap, min(g.size + k, g.cap)
        n_alive[r] = int((~done).sum())
        alive_next_obs[r, :n_alive[r]] = next_obs[r, :k][~done]
        sums[r] = ordered_sum(rew[r, :k])
    return n_alive, sums

"""GPU: the rollout append of csrc/store.hip -- orl_buffer_append_rollout_runs and orl_buffer_append_rollout, which share one host path
and one device core -- against the numpy oracle tests/store_refs.py: ring contents, survivors and untouched cells as bit patterns, the
float64 reward sums equal (the oracle adds in the device's order)."""
import functools

import numpy as np
import pytest
import torch

import store_refs as sr
from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R, CAP, STRIDE = 3, 320, 300
CALLS = ((300, 257, 0), (256, 1, 44))       # run 0 wraps inside its first block on the second call; blocks of 44 and 1 rows; an empty run


@functools.lru_cache(maxsize=None)
def _inputs():
    """the fixture's rows arange(STRIDE) % 368 for every run (27 observation columns -> pitch 28, 3 action columns -> pitch 4) and
    per-call, per-run rewards"""
    g = load_golden("mb_termination")
    rows = np.arange(STRIDE) % len(g["obs"])
    obs, act, nxt = (np.broadcast_to(g[k][rows], (R, STRIDE, g[k].shape[1])).copy() for k in ("obs", "act", "next_obs"))
    assert np.isnan(nxt).any()
    rng = np.random.RandomState(7)
    return obs, act, nxt, [rng.standard_normal((R, STRIDE)).astype(np.float32) * 3.0 for _ in CALLS]


@functools.lru_cache(maxsize=None)
def _oracle(kind):
    """per call: (n_alive, sums, alive_next_obs, the columns of the R rings after it)"""
    obs, act, nxt, rews = _inputs()
    rings = [sr.Ring(CAP, obs.shape[2], act.shape[2]) for _ in range(R)]
    out = []
    for n, rew in zip(CALLS, rews):
        alive = np.full(nxt.shape, -7.0, np.float32)
        n_alive, sums = sr.append_rollout(rings, kind, obs, act, nxt, rew, n, alive)
        out.append((n_alive, sums, alive, [[c.copy() for c in g.columns()] for g in rings], [g.size for g in rings]))
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("kind", ["TERM_ANT", "TERM_WALKER2D", "TERM_PEN", "TERM_NONE"])
def test_append_rollout_both_entry_points_equal_the_oracle(kind):
    from offlinerlkit import _engine
    k = getattr(sr, kind)
    obs, act, nxt, rews = _inputs()
    od, ad = obs.shape[2], act.shape[2]
    t = lambda x: torch.tensor(x, device=DEV)
    rings = [_engine.DeviceBuffer(od, ad) for _ in range(R)]
    single = _engine.DeviceBuffer(od, ad)          # run 0's rows through the single-ring entry point
    for b in rings + [single]:
        b.reserve(CAP)
    d_obs, d_act, d_nxt = t(obs), t(act), t(nxt)
    try:
        for n, rew, (want_alive, want_sums, want_nobs, want_rings, want_sizes) in zip(CALLS, rews, _oracle(k)):
            d_rew = t(rew)
            alive = torch.full((R, STRIDE, od), -7.0, device=DEV)
            n_alive, sums = _engine.DeviceBuffer.append_rollout_runs(rings, k, d_obs, d_act, d_nxt, d_rew, n, alive)
            alive1 = torch.full((n[0], od), -7.0, device=DEV)
            na1, s1 = single.append_rollout(k, d_obs[0, :n[0]], d_act[0, :n[0]], d_nxt[0, :n[0]], d_rew[0, :n[0]], alive1)
            for r in range(R):
                print(f"{kind} n={n[r]}: n_alive {n_alive[r]} (oracle {want_alive[r]}) sum {sums[r]!r} (oracle {want_sums[r]!r})")
            print(f"{kind} single n={n[0]}: n_alive {na1} sum {s1!r}")
            # not vacuous (the oracle's counts are pinned to the fixture in test_store_refs_cpu.py)
            for r in range(R):
                if kind == "TERM_NONE":
                    assert want_alive[r] == n[r]
                elif n[r] >= 44:
                    assert 0 < want_alive[r] < n[r], (r, want_alive[r])
            assert np.array_equal(n_alive, want_alive) and n_alive.dtype == np.int64
            assert np.array_equal(_bits(sums), _bits(want_sums)) and all(sums[r] == want_sums[r] for r in range(R))
            assert np.array_equal(_bits(alive.cpu().numpy()), _bits(want_nobs))          # survivors, and the sentinel behind them
            assert na1 == want_alive[0] and s1 == want_sums[0]
            assert np.array_equal(_bits(alive1.cpu().numpy()), _bits(want_nobs[0, :n[0]]))
            for b, want, size in zip(rings + [single], want_rings + [want_rings[0]], want_sizes + [want_sizes[0]]):
                assert b.size() == size
                for got, col in zip(b.read_rows(0, CAP), want):
                    assert np.array_equal(_bits(got), _bits(col))
    finally:
        for b in rings + [single]:
            b.close()

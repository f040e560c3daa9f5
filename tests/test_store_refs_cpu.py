"""CPU: the numpy oracle of the rollout append (tests/store_refs.py) against plain numpy -- its verdicts against
utils/termination_fns.py and the reference's recorded ones, its ordered float64 sum against math.fsum, its ring against a row loop."""
import math

import numpy as np
import pytest

import store_refs as sr
from helpers import load_golden

KIND_FN = {"TERM_NONE": "default", "TERM_HALFCHEETAH": "halfcheetah", "TERM_HOPPER": "hopper", "TERM_WALKER2D": "walker2d",
           "TERM_ANT": "ant", "TERM_HUMANOID": "humanoid", "TERM_PEN": "pen"}
# rows of the fixture done among its first 44 / 256 / 257 / 300: the shapes test_gpu_store.py runs keep some rows and lose some
DONE_COUNTS = {"TERM_ANT": (33, 141, 141, 145), "TERM_WALKER2D": (40, 224, 225, 268), "TERM_PEN": (24, 32, 32, 32)}


@pytest.mark.parametrize("kind", sorted(KIND_FN))
def test_verdicts_equal_the_termination_functions(kind):
    from offlinerlkit.utils import termination_fns as T
    g = load_golden("mb_termination")
    obs, act, nxt = g["obs"], g["act"], g["next_obs"]
    assert np.isnan(nxt).any() and np.isinf(nxt).any()
    assert getattr(sr, kind) == getattr(T, kind)
    got = sr.term_done(getattr(sr, kind), nxt)
    assert got.dtype == bool and got.shape == (len(nxt),)
    for want in (getattr(T, "termination_fn_" + KIND_FN[kind])(obs, act, nxt), g["fn_" + KIND_FN[kind]]):
        want = np.asarray(want).astype(bool).ravel()
        assert np.array_equal(got.astype(np.float32).view(np.uint32), want.astype(np.float32).view(np.uint32)), kind
    if kind in DONE_COUNTS:
        assert tuple(int(got[:k].sum()) for k in (44, 256, 257, 300)) == DONE_COUNTS[kind]


@pytest.mark.parametrize("n", [0, 1, 44, 63, 64, 65, 256, 257, 600])
def test_ordered_sum_is_a_float64_sum(n):
    rew = np.linspace(-3, 5, 600).astype(np.float32)[:n]
    got = sr.ordered_sum(rew)
    assert isinstance(got, np.float64)
    exact = math.fsum(float(x) for x in rew)
    print(f"n={n}: ordered {got!r} fsum {exact!r} np.sum {rew.astype(np.float64).sum()!r}")
    assert abs(got - exact) <= 1e-9 * float(np.abs(rew).astype(np.float64).sum())
    if n <= 1:
        assert got == (float(rew[0]) if n else 0.0)


def test_ordered_sum_order():
    """the order itself, on values whose float64 sum depends on it: 2^60 in lane 0, -2^60 in lane 32 (they meet in the first tree
    step and cancel), ones elsewhere; and in lanes 0 and 1 (they meet in the last step, after the ones were absorbed by 2^60)"""
    v = np.ones(64, np.float32)
    v[0], v[32] = 2.0 ** 60, -2.0 ** 60
    assert sr.ordered_sum(v) == 62.0
    v = np.ones(64, np.float32)
    v[0], v[1] = 2.0 ** 60, -2.0 ** 60
    assert sr.ordered_sum(v) == 0.0
    # waves: ((w0 + w1) + w2) + w3; blocks: in order
    w = np.zeros(256, np.float32)
    w[0], w[64], w[128], w[192] = 1.0, 2.0 ** 60, -2.0 ** 60, 1.0
    assert sr.ordered_sum(w) == 1.0
    b = np.zeros(3 * 256, np.float32)
    b[0], b[256], b[512] = 2.0 ** 60, 1.0, -2.0 ** 60
    assert sr.ordered_sum(b) == 0.0


def test_append_rollout_wraps_compacts_and_takes_empty_runs():
    g = load_golden("mb_termination")
    od, ad, cap, stride, R = 27, 3, 320, 300, 3
    rows = np.arange(stride) % len(g["obs"])
    obs, act, nxt = (np.broadcast_to(g[k][rows], (R, stride, g[k].shape[1])).copy() for k in ("obs", "act", "next_obs"))
    rng = np.random.RandomState(0)
    rings = [sr.Ring(cap, od, ad) for _ in range(R)]
    loop = [dict(o=[], a=[], no=[], r=[], t=[]) for _ in range(R)]          # every appended row, in order
    done = sr.term_done(sr.TERM_ANT, g["next_obs"][rows])
    for n in ((300, 257, 0), (256, 1, 44)):
        rew = rng.standard_normal((R, stride)).astype(np.float32)
        alive = np.full((R, stride, od), -7.0, np.float32)
        n_alive, sums = sr.append_rollout(rings, sr.TERM_ANT, obs, act, nxt, rew, n, alive)
        for r in range(R):
            k = n[r]
            assert n_alive[r] == (~done[:k]).sum() and (k < 44 or 0 < n_alive[r] < k)
            assert np.array_equal(alive[r, :n_alive[r]].view(np.uint32), nxt[r, :k][~done[:k]].view(np.uint32))
            assert (alive[r, n_alive[r]:] == -7.0).all()
            assert sums[r] == sr.ordered_sum(rew[r, :k]) and (k > 0 or sums[r] == 0.0)
            for key, v in zip(("o", "a", "no", "r", "t"), (obs[r, :k], act[r, :k], nxt[r, :k], rew[r, :k, None], done[:k, None])):
                loop[r][key].extend(v)
    assert [(b.ptr, b.size) for b in rings] == [(236, 320), (258, 258), (44, 44)]
    for r, b in enumerate(rings):
        total = len(loop[r]["r"])
        for key, col in zip(("o", "a", "no", "r", "t"), b.columns()):
            want = np.zeros_like(col)
            for i in range(total):                                           # later rows overwrite earlier ones
                want[i % cap] = loop[r][key][i]
            assert np.array_equal(col.view(np.uint32), want.view(np.uint32)), (r, key)

"""GPU: step_head = 1 (k_dyn_head_tile) against float64 and against k_dyn_head.

Two engines of one config, parameter block, scaler and elites, step_head 0 and 1, on the same obs / act / noise / member indices in the
three penalty modes.  (a) the step_head = 1 outputs are held to dyn_refs.head in float64 on that engine's own ``step.out`` tap by the
bounds of test_gpu_dyn_kernels.test_step (tests/row_refs.py); (b) every output of the two engines has the same bits.
Cases (tests/dyn_cases.py): n = 1, 15, 16, 17, 37 at BASE (one row, the tail of a 16-row tile, a full tile, a second tile), D = 2, one
member, the last member as the only elite, two runs (the run offsets of max / min_logvar and the elites), precision 1, and 64 members at
od = 12 / 20 / 39 / 63, where the LDS image allows 8 / 4 / 2 / 1 rows a tile.  The last test draws on the device (n = 300, two runs).
"""
import numpy as np
import pytest

import dyn_cases as dc
import dyn_refs as dr
import test_gpu_dyn_kernels as tk

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = [("n%d" % n, dc.case(), n, 0) for n in (1, 15, 16, 17, 37)] + \
        [(k, dc.SHAPES[k], 37, 0) for k in ("od1", "K1", "elite_last")] + [("runs2", dc.case(R=2), 37, 0), ("p1", dc.case(), 37, 1)] + \
        [("K64_od%d" % od, dc.case(od=od, ad=2, **dc.K64), 37, 0) for od in (12, 20, 39, 63)]


def make2(c, seed, precision=0):
    """tk.make's engine (step_head 0) as x.eng and one with step_head = 1 as x.tile: same parameters, scalers and elites"""
    from offlinerlkit import _engine
    x = tk.make(c, seed)
    engs = []
    for sh in (0, 1):
        cfg = type(x.cfg).from_buffer_copy(x.cfg)
        cfg.precision, cfg.step_head = precision, sh
        engs.append(_engine.Dynamics(cfg))
        for r in range(x.R):
            engs[sh].set_params(r, x.st[r]), engs[sh].set_scaler(r, x.mu[r], x.sd[r]), engs[sh].set_elites(r, list(c["elites"]))
    x.eng.close()
    x.eng, x.tile = engs
    assert (x.eng.step_head, x.tile.step_head) == (0, 1)
    return x


def same(a, b, tag):
    for name, u, v in zip(("next_obs", "reward", "raw_reward", "penalty", "midx_out"), a, b):
        dr.same_bits(np.asarray(u).astype(f32), np.asarray(v).astype(f32), tag + (name, "step_head 1 against 0"))


@pytest.mark.parametrize("cid,c,n,prec", CASES, ids=[t[0] for t in CASES])
def test_tile_head(cid, c, n, prec):
    x = make2(c, seed=7 * len(cid) + n, precision=prec)
    rng, R, K, D = x.rng, x.R, x.K, x.D
    obs, act = tk.inputs(x, rng, n)
    for mode in dr.MODES:
        noise = rng.normal(size=(R, K, n, D)).astype(f32)
        midx = rng.choice(np.asarray(c["elites"]), size=(R, n))
        old, new = x.eng.step(obs, act, noise, midx, mode, 2.5), x.tile.step(obs, act, noise, midx, mode, 2.5)
        nxt, rew, raw, pen, mo = new
        assert (mo == midx).all()
        for r in range(R):
            tg = ("tile", cid, mode, r)
            st, out = x.st[r], x.tile.debug_read(r, "step.out")
            ref = dr.head(out, obs[r], noise[r], midx[r], st["max_logvar"], st["min_logvar"], mode, 2.5)
            tk.holds(nxt[r], ref[0], "k_dyn_head.next_obs", *tg), tk.holds(raw[r], ref[1], "k_dyn_head.raw_reward", *tg)
            tk.holds(pen[r], ref[2], "k_dyn_head.penalty." + mode, *tg), tk.holds(rew[r], ref[3], "k_dyn_head.reward", *tg)
        same(new, old, ("tile", cid, mode))
    x.eng.close(), x.tile.close()


def test_tile_head_device_draws():
    """no noise, no indices: both engines draw from Philox at the same seed and call counter, so equal bits mean equal counter words"""
    c = dc.case(R=2)
    x = make2(c, seed=5)
    obs, act = tk.inputs(x, x.rng, 300)
    for mode in dr.MODES:
        old, new = x.eng.step(obs, act, None, None, mode, 1.0), x.tile.step(obs, act, None, None, mode, 1.0)
        assert np.isin(new[4], c["elites"]).all() and len(np.unique(new[4])) > 1
        same(new, old, ("tile device draws", mode))
    x.eng.close(), x.tile.close()

"""GPU: the dynamics ensemble at precision 1 (csrc/dynamics_fused.hip: k_dyn_pack_planes + k_dyn_fused_fwd under step / sample_next).

``step.out`` of every run against a float64 numpy forward of the engine's own ``step.x``.  Bar: scale_err(got, o64)
<= SPLIT x BAR x D32 = 16 x D32, D32 = scale_err(o32, o64) of the same forward in fp32, each over a run's whole [K][n][2D] tensor.  A
CPU emulation of the three-product split gave at most 4.5 x D32; a dropped cross term or lo plane lands above 380 x D32.
Cases, one edge each from dyn_cases.BASE: rows 1 .. 257 (tails of the 16-row tile, several tiles), 2801 and 5505 (the 32- and 64-row
tiles: 88 x 3 and 87 x 3 >= 256 workgroups, tails of 17 rows and of 1), widths 20 / 36 (K tail, partial fragment), the workload's
[200] x 4 x 7 members at 65, 1185 and 2369 rows (all three tiles), 256 and the limit 512 (8 fragments per wave), in = 2 and 65, K = 1,
two runs.  Every case prints its err / D32 (MI355X: profiles/dyn_step_split_accuracy.json).
"""
import numpy as np
import pytest

import dyn_cases as dc
import dyn_refs as dr
import test_gpu_dyn_kernels as tk
from helpers import scale_err

pytestmark = pytest.mark.gpu
f32 = np.float32
BAR = 16.0                                  # SPLIT (4) x BAR (4) of tests/diffusion_split_cases.py
WORK = dict(od=17, ad=6, K=7, elites=(6, 1, 2, 3, 0), hidden=(200,) * 4, decays=(0.0,) * 5)
ONE = dict(decays=(0.1, 5e-4))
CASES = [("n%d" % n, dc.case(), n) for n in (1, 15, 16, 17, 63, 65, 257, 2801, 5505)] + [
    ("h20_36", dc.case(hidden=(20, 36)), 65),
    ("work", dc.case(**WORK), 65), ("work_rt32", dc.case(**WORK), 1185), ("work_rt64", dc.case(**WORK), 2369),
    ("h256", dc.case(hidden=(256,), **ONE), 17), ("h512", dc.case(hidden=(512,), **ONE), 17),
    ("od1", dc.case(od=1, ad=1), 65), ("od63", dc.case(od=63, ad=2), 65), ("K1", dc.case(K=1, elites=(0,)), 65), ("R2", dc.case(R=2), 65),
]


def make1(c, seed):
    """tk.make's precision-0 engine x.eng and a precision-1 engine x.eng1 with the same parameters, scalers and elites"""
    from offlinerlkit import _engine
    x = tk.make(c, seed)
    cfg = type(x.cfg).from_buffer_copy(x.cfg)
    cfg.precision = 1
    x.eng1 = _engine.Dynamics(cfg)
    assert (x.eng.precision, x.eng1.precision) == (0, 1)
    for r in range(x.R):
        x.eng1.set_params(r, x.st[r]), x.eng1.set_scaler(r, x.mu[r], x.sd[r]), x.eng1.set_elites(r, list(c["elites"]))
    return x


def forward(X, st, dt):
    """[K, n, 2D]: the ensemble's forward of the rows X [n, in] in dtype dt"""
    h = np.asarray(X, dt)[None]
    L = len([k for k in st if k.startswith("backbones.") and k.endswith(".weight")])
    for l in range(L + 1):
        pre = "backbones.%d." % l if l < L else "output_layer."
        h = np.matmul(h, st[pre + "weight"].astype(dt)) + st[pre + "bias"].astype(dt)
        if l < L:
            h = h / (1 + np.exp(-h))
    assert h.dtype == dt
    return h


def step(x, eng, obs, act, seed=0):
    rng = np.random.default_rng(seed)
    noise = rng.normal(size=(x.R, x.K, obs.shape[1], x.D)).astype(f32)
    midx = rng.choice(np.asarray(x.c["elites"]), size=obs.shape[:2])
    return eng.step(obs, act, noise, midx, "aleatoric", 1.0)


def out_ratio(x, eng, obs, act, tag):
    """step.x bit for bit, step.out of every run against float64: the worst err / D32"""
    worst = 0.0
    for r in range(x.R):
        X, out = eng.debug_read(r, "step.x"), eng.debug_read(r, "step.out")
        dr.same_bits(X, dr.scale_rows(np.concatenate([obs[r], act[r]], 1), x.mu[r], x.sd[r]), tag + (r, "step.x"))
        o64, o32 = forward(X[:, :x.n_in], x.st[r], np.float64), forward(X[:, :x.n_in], x.st[r], f32)
        assert out.shape == o64.shape
        d32 = scale_err(o32, o64)
        assert d32 > 0.0, tag
        worst = max(worst, scale_err(out, o64) / d32)
    print(f"{tag}: worst err / D32 {worst:.2f} (bar {BAR:.0f})")
    return worst


@pytest.mark.parametrize("cid,c,n", CASES, ids=[t[0] for t in CASES])
def test_step_out_vs_float64(cid, c, n):
    x = make1(c, seed=len(cid) + n)
    obs, act = tk.inputs(x, x.rng, n)
    step(x, x.eng1, obs, act)
    assert out_ratio(x, x.eng1, obs, act, ("fused", cid, n)) <= BAR
    x.eng.close(), x.eng1.close()


@pytest.mark.parametrize("n,S", [(65, 3), (1, 1)])
def test_sample_next(n, S):
    c = dc.case()
    x = make1(c, seed=n)
    obs, act = tk.inputs(x, x.rng, n)
    noise = x.rng.normal(size=(1, S, len(c["elites"]), n, x.D)).astype(f32)
    got = x.eng1.sample_next(obs, act, S, noise)
    assert out_ratio(x, x.eng1, obs, act, ("fused sample_next", n, S)) <= BAR
    st = x.st[0]
    tk.holds(got[0], dr.sample_next(x.eng1.debug_read(0, "step.out"), obs[0], noise[0], c["elites"], st["max_logvar"], st["min_logvar"]),
             "k_dyn_sample_next.next_obs", "fused sample_next", n, S)
    x.eng.close(), x.eng1.close()


def test_option_does_not_leak():
    """training and validation are the fp32 arithmetic at either precision, bit for bit; only the step differs"""
    x = make1(dc.case(), seed=3)
    data_in, data_tg = (3.0 * x.rng.normal(size=(50, x.n_in))).astype(f32), x.rng.normal(size=(50, x.D)).astype(f32)
    idx, hold = x.rng.integers(0, 50, size=(1, x.K, 100)), x.rng.integers(0, 50, size=(1, 33))
    flat = []
    for eng in (x.eng, x.eng1):
        eng.load_data(data_in, data_tg)
        loss, mse = eng.learn_epoch(idx), eng.validate(hold)
        flat.append(np.concatenate([x.flatten(eng.get_params(0)), loss, mse.ravel()]))
    dr.same_bits(flat[1], flat[0], ("learn_epoch + validate", "precision 1 against 0"))
    assert (flat[0][:x.eng.P] != x.flat[0]).any()
    x.st[0] = x.eng.get_params(0)
    obs, act = tk.inputs(x, x.rng, 65)
    out = []
    for eng in (x.eng, x.eng1):
        step(x, eng, obs, act)
        out.append(eng.debug_read(0, "step.out"))
    assert (out[0].view(np.uint32) != out[1].view(np.uint32)).any()
    assert out_ratio(x, x.eng1, obs, act, ("fused after learn_epoch",)) <= BAR
    x.eng.close(), x.eng1.close()


def test_refusals_and_range_flags():
    from offlinerlkit import _engine
    for over, msg in ((dict(precision=2), "precision 2"), (dict(precision=1, hidden=[513]), "at most 512")):
        with pytest.raises(RuntimeError, match=msg):
            _engine.Dynamics(_engine.default_dyn_config(obs_dim=3, act_dim=2, **over))
    x = make1(dc.case(), seed=9)
    eng = x.eng1
    obs, act = tk.inputs(x, x.rng, 17)
    good = step(x, eng, obs, act)

    def same_as_before():
        for a, b in zip(step(x, eng, obs, act), good):
            dr.same_bits(a.astype(f32), b.astype(f32), ("step after a range flag",))

    eng.set_scaler(0, x.mu[0], np.full(x.n_in, 1e-2, f32))
    with pytest.raises(RuntimeError, match="range flag.*activation"):
        step(x, eng, np.full_like(obs, 1e3), act)
    eng.set_scaler(0, x.mu[0], x.sd[0])
    same_as_before()
    w = {k: v.copy() for k, v in x.st[0].items()}
    w["backbones.1.weight"][-1, -1, -1] = 2000.0
    eng.set_params(0, w)
    for _ in range(2):                               # sticky for as long as the weight stays
        with pytest.raises(RuntimeError, match="range flag.*weight"):
            step(x, eng, obs, act)
    eng.set_params(0, x.st[0])
    same_as_before()
    x.eng.close(), eng.close()


def test_ensemble_dynamics_option():
    """EnsembleDynamics.set_engine_options(precision=1): step_device is the precision-1 engine's step at the same call counter"""
    import torch
    from offlinerlkit import _engine
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.modules import EnsembleDynamicsModel
    from offlinerlkit.utils.scaler import StandardScaler
    rng = np.random.default_rng(5)
    mu, sd = dc.scaler(rng, 5)
    obs, act = torch.randn(65, 3, device="cuda"), torch.randn(65, 2, device="cuda")
    got = {}
    for prec in (0, 1):
        torch.manual_seed(1)
        m = EnsembleDynamicsModel(3, 2, [32, 32], 3, 2, weight_decays=[0.0, 0.1, 5e-4])
        dyn = EnsembleDynamics(m, None, StandardScaler(mu, sd), None, penalty_coef=1.0)
        if prec:
            dyn.set_engine_options(precision=1)
        nxt, rew, info = dyn.step_device(obs, act)
        assert dyn._eng.precision == prec
        got[prec] = torch.cat([nxt, rew[:, None], info["penalty"][:, None]], 1).cpu().numpy()
    params = {k: v.detach().cpu().numpy() for k, v in m.named_parameters() if k != "elites"}
    eng = _engine.Dynamics(_engine.default_dyn_config(obs_dim=3, act_dim=2, hidden=[32, 32], num_ensemble=3, num_elites=2,
                                                      weight_decay=[0.0, 0.1, 5e-4], precision=1))
    eng.set_params(0, params), eng.set_scaler(0, mu, sd), eng.set_elites(0, m.elites.detach().cpu().numpy())
    nxt, rew, raw, pen = eng.step_device(obs[None].contiguous(), act[None].contiguous(), "aleatoric", 1.0)
    dr.same_bits(got[1], torch.cat([nxt[0], rew[0][:, None], pen[0][:, None]], 1).cpu().numpy(), ("EnsembleDynamics.step_device",))
    assert (got[0] != got[1]).any()
    eng.close()

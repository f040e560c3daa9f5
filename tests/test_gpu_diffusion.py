"""GPU: DiffusionBC on the engine (orl_diffusion_*) against the reference fixtures of tests/golden/make_diffusion_golden.py, the numpy
oracle and float64 autograd; the policy class on top of it; ``RcslPolicy.rollout_device`` with its frozen noise.

Bars: output and loss 1e-4 (scale_err / rel_err with floor 1e-2, the project's gate); gradients 4 x the distance the reference's fp32
autograd shows from float64 autograd on the same batch, measured by the generator and stored in the fixture, in the norm of
diffusion_oracle.grad_distance (the 4 covers another summation order in the GEMMs and the group statistics); the 20-step trajectory, the final parameters and the final EMA K = 4 x the reference's own one-ulp twin
(tests/long_horizon.py's rule); sampling 1e-4 of scale."""
import numpy as np
import pytest
import torch
from scipy import stats

import diffusion_cases as dc
import diffusion_oracle as orc
import long_horizon as lh
from helpers import load_golden, rel_err, scale_err
from diffusion_oracle import grad_distance

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def shapes_of(c):
    from offlinerlkit.nets import ConditionalUnet1D
    net = ConditionalUnet1D(c["act_dim"], c["obs_dim"], **dc.net_kwargs(c))
    return net, [(k, tuple(v.shape)) for k, v in net.state_dict().items()]


def pack(eng, P):
    flat = np.zeros(eng.floats, np.float32)
    for name, off, shape in eng.tensors():
        t = P[name]
        if t.ndim == 3:
            t = t[:, :, t.shape[2] // 2]
        assert t.shape == shape, (name, t.shape, shape)
        flat[off:off + t.size] = t.ravel()
    return flat


def unpack(eng, flat, like):
    """{key: array of the state_dict shape}; the off-centre taps come from ``like``"""
    out = {k: np.array(v, copy=True) for k, v in like.items()}
    for name, off, shape in eng.tensors():
        t = flat[off:off + int(np.prod(shape))].reshape(shape)
        if out[name].ndim == 3:
            out[name][:, :, out[name].shape[2] // 2] = t
        else:
            out[name][...] = t
    return out


def make_engine(c, total_steps=20, seed=0, B=None):
    from offlinerlkit import _engine
    from offlinerlkit.policy.diffusion import ddpm_schedule, lr_table
    cfg = _engine.default_diffusion_config(obs_dim=c["obs_dim"], act_dim=c["act_dim"], step_embed_dim=c["dsed"], down_dims=c["down_dims"],
                                           kernel_size=c["kernel_size"], n_groups=c["n_groups"], num_diffusion_iters=c["N"],
                                           batch_size=B or c["B"], seed=seed)
    eng = _engine.Diffusion(cfg)
    _, acp, coef = ddpm_schedule(c["N"])
    eng.set_schedule(acp, coef)
    eng.set_lr(lr_table(total_steps))
    _, shapes = shapes_of(c)
    P = dc.make_params(c, shapes)
    flat = pack(eng, P)
    eng.set(eng.PARAMS, flat)
    eng.set(eng.EMA, flat)
    obs, act = dc.make_data(c)
    buf = _engine.DeviceBuffer(c["obs_dim"], c["act_dim"])
    z = np.zeros(len(obs), np.float32)
    buf.load(obs, act, obs, z, z)
    eng.attach_buffer(buf)
    return eng, P


def zero_like_grads(eng, P):
    return unpack(eng, eng.debug_grads(), {k: np.zeros_like(v) for k, v in P.items()})


# ---- 1. one step on fixture (a) -----------------------------------------------------------------------------------------------------------
def test_step_matches_the_reference_fixture():
    c = dc.CASES["a"]
    g = load_golden("diffusion_a")
    eng, P = make_engine(c)
    try:
        idx, t, eps = dc.make_steps(c, 1)[0]
        loss = eng.step(idx, t, eps)
        pred = eng.debug_read("pred").reshape(len(idx), c["act_dim"])
        print(f"(a) loss {loss!r} vs {float(g['loss'])!r}; pred scale_err {scale_err(pred, g['pred']):.2e}")
        assert np.array_equal(eng.debug_read("eps").reshape(eps.shape), eps) and np.array_equal(eng.debug_read("t"), t.astype(np.float32))
        assert scale_err(eng.debug_read("x_t").reshape(pred.shape), g["x_t"]) < 1e-6
        assert scale_err(pred, g["pred"]) < 1e-4
        assert rel_err(np.array([loss]), np.array([g["loss"]]), floor=1e-2) < 1e-4
        assert eng.debug_read("loss")[0] == np.float32(loss) and eng.step_count == 1
        # gradients: the three tensors that have one against float64 autograd, the structurally zero ones against the fp32 noise
        got = zero_like_grads(eng, P)
        g64 = {k[len("grad64/"):]: g[k] for k in g.files if k.startswith("grad64/")}
        assert sorted(g64) == ["final_conv.0.block.1.bias", "final_conv.1.bias", "final_conv.1.weight"]
        D, noise = float(g["grad_f32_vs_f64"]), float(g["grad_zero_noise"])
        for k, v in g64.items():
            e = np.abs(got[k] - v).max() / np.abs(v).max()
            print(f"    grad {k}: {e:.2e} (bound {4 * D:.2e})")
            assert e <= 4 * D, (k, e, D)
        worst = max(np.abs(v).max() for k, v in got.items() if k not in g64)
        print(f"    largest |gradient| on the structurally zero tensors: {worst:.2e} (fp32 autograd: {noise:.2e})")
        assert worst <= 4 * noise
        # the first step has lr 0: Adam moves nothing, the EMA (decay 0) equals the parameters
        assert np.array_equal(eng.get(eng.PARAMS), pack(eng, P)) and np.array_equal(eng.get(eng.EMA), pack(eng, P))
    finally:
        eng.close()


# ---- 2. every tensor's gradient: the reference's nets without a one-channel group ---------------------------------------------------------
def centre_taps(G):
    return {k: (v[:, :, v.shape[2] // 2] if v.ndim == 3 else v) for k, v in G.items()}


def _check_batch(eng, P, c, batch, g, tag, what):
    """one engine step on ``batch`` against a fixture's pred / loss / float64 gradients under ``tag``; the gradient bar is 4 x the
    distance the reference's own fp32 autograd showed on this batch (stored by the generator)"""
    idx, t, eps = batch
    loss = eng.step(idx, t, eps)
    pred = eng.debug_read("pred").reshape(len(idx), c["act_dim"])
    got = zero_like_grads(eng, P)
    for k, v in got.items():                           # the off-centre taps: exactly zero
        if v.ndim == 3 and v.shape[2] > 1:
            assert not np.delete(v, v.shape[2] // 2, axis=2).any()
    g64 = {k[len(tag) + 7:]: g[k] for k in g.files if k.startswith(tag + "grad64/")}
    assert sorted(g64) == sorted(P)
    D = float(g[tag + "grad_f32_vs_f64"])
    Dg, noise = grad_distance(centre_taps(got), g64)
    print(f"{what}: loss {loss!r} (reference {float(g[tag + 'loss'])!r}); pred {scale_err(pred, g[tag + 'pred']):.2e}; "
          f"gradients {Dg:.2e}, reference fp32 autograd {D:.2e}")
    assert noise == 0.0                                 # every tensor has a gradient
    assert scale_err(eng.debug_read("x_t").reshape(pred.shape), g[tag + "x_t"]) < 1e-6
    assert scale_err(pred, g[tag + "pred"]) < 1e-4 and rel_err(np.array([loss]), np.array([g[tag + "loss"]]), floor=1e-2) < 1e-4
    assert np.ptp(g[tag + "pred"], axis=0).max() > 0.1  # the output depends on the row: the body of the net is in the check
    assert Dg <= 4 * D, (Dg, D)


@pytest.mark.parametrize("step", [0, 1])
def test_every_gradient_against_the_reference(step):
    """fixture (d), groups of 3 and 4 channels: the full batch (step 0) and the short last batch of 2 rows (step 1)"""
    c = dc.CASES["d"]
    eng, P = make_engine(c)
    try:
        batch = dc.make_steps(c, 2)[step]
        assert len(batch[0]) == (6, 2)[step]
        _check_batch(eng, P, c, batch, load_golden("diffusion_d"), f"b{step}/", f"(d) batch {step}")
    finally:
        eng.close()


def test_block_groups_other_than_eight():
    """fixture (e): n_groups = 4 in the blocks, GroupNorm(8) in final_conv as the reference builds it"""
    c = dc.CASES["e"]
    eng, P = make_engine(c)
    try:
        _check_batch(eng, P, c, dc.make_steps(c, 1)[0], load_golden("diffusion_e"), "", "(e)")
    finally:
        eng.close()


# ---- 3. the 20-step trajectory of (b) --------------------------------------------------------------------------------------------------------
def _param_dev(x, ref):
    """the largest |x - ref| / max(|ref|, 1 % of the tensor's scale) over every tensor"""
    return max(float((np.abs(x[k].astype(np.float64) - ref[k]) / np.maximum(np.abs(ref[k]), 1e-2 * np.abs(ref[k]).max())).max()) for k in ref)


@pytest.mark.parametrize("name", ["b", "d"])
def test_trajectory_stays_inside_the_twin_envelope(name):
    """(b): 20 steps of the issue's net, where only final_conv trains; (d): 12 steps of the net whose every tensor trains"""
    c = dc.CASES[name]
    g = load_golden("diffusion_b" if name == "b" else "diffusion_d_traj")
    steps = dc.make_steps(c, c["steps"])
    assert {len(s[0]) for s in steps} == {6, 2}                       # the short last batch of every epoch is included
    eng, P = make_engine(c, total_steps=c["steps"])
    try:
        losses = np.array([eng.step(*s) for s in steps], np.float64)
        ref, twin = g["losses"][:, None], g["losses_twin"][:, None]
        d = np.maximum.accumulate(lh.deviation(losses[:, None], ref))
        env = lh.envelope(ref, [twin])
        for T in (5, 10, c["steps"]):
            print(f"({name}) loss deviation by step {T}: {d[T - 1]:.2e} (twin envelope {env[T - 1]:.2e})")
            assert d[T - 1] <= lh.K_ENVELOPE * env[T - 1], (T, d[T - 1], env[T - 1])
        assert d[-1] < 1e-4
        for tag, which in (("final", eng.PARAMS), ("ema", eng.EMA)):
            got = unpack(eng, eng.get(which), P)
            want = {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + "/")}
            tw = {k[len(tag) + 6:]: g[k] for k in g.files if k.startswith(tag + "_twin/")}
            if name == "d":                                            # (d) stores the centre taps
                got = centre_taps(got)
            dev, env_p = _param_dev(got, want), _param_dev(tw, want)
            print(f"    {tag}: deviation {dev:.2e} (twin {env_p:.2e})")
            assert dev <= lh.K_ENVELOPE * env_p, (tag, dev, env_p)
            if tag == "final" and name == "b":                         # the reference's off-centre taps never move (its EMA of them
                for k, v in want.items():                              # rounds: ema d + p (1 - d) of a constant is not the constant)
                    if v.ndim == 3 and v.shape[2] > 1:
                        assert np.array_equal(np.delete(v, v.shape[2] // 2, axis=2), np.delete(P[k], v.shape[2] // 2, axis=2))
        if name == "d":
            moved = [k for k, v in centre_taps(unpack(eng, eng.get(eng.PARAMS), P)).items() if not np.array_equal(v, centre_taps(P)[k])]
            assert len(moved) == len(P)                                # every tensor trained
    finally:
        eng.close()


# ---- 4. sampling -------------------------------------------------------------------------------------------------------------------------------
def test_sampling_matches_the_reference_and_the_oracle():
    g = load_golden("diffusion_c")
    for name in ("c", "d"):
        c = dict(dc.CASES[name], rows=4)
        eng, P = make_engine(c)
        try:
            obs, noise, z = dc.make_sample_inputs(c)
            got = eng.sample(obs, noise.reshape(4, -1), z=z)
            want = g["actions"] if name == "c" else load_golden("diffusion_d")["actions"]      # both from the reference's module
            assert scale_err(orc.sample(P, c, obs, noise, z), want) < 1e-5
            print(f"({name}) sampled actions: scale_err {scale_err(got, want):.2e}")
            assert scale_err(got, want) < 1e-4
            one = eng.sample(obs[:1], noise.reshape(4, -1)[:1], z=z[:, :1])
            assert np.array_equal(one[0], got[0])                      # a one-row call is row 0 of the batched call
            # gathered frozen noise: row i reads noise row idx[i]
            pick = np.array([2, 0, 3, 1], np.int64)
            gathered = eng.sample(obs[pick], noise.reshape(4, -1), noise_idx=pick, z=z[:, pick])
            assert np.array_equal(gathered, got[pick])
            assert eng.step_count == 0                                  # sampling moves neither the step counter nor the parameters
            assert np.array_equal(eng.get(eng.PARAMS), pack(eng, P))
        finally:
            eng.close()


# ---- 5. the device draws ----------------------------------------------------------------------------------------------------------------------
def test_device_draws_are_uniform_and_standard_normal():
    """t by the chi-square rule of test_gpu_learn_n's samplers, eps and z by its ``_moments_ok`` (mean, variance, skew, excess kurtosis
    at 5 sigma) and its KS rule (p > 1e-3)"""
    from test_gpu_learn_n import _moments_ok
    c = dict(dc.CASES["b"])
    B, calls = 4096, 8
    eng, P = make_engine(c, total_steps=calls, B=B)
    try:
        idx = (np.arange(B) % c["n"]).astype(np.int64)
        ts, es = [], []
        for _ in range(calls):
            eng.step(idx)
            ts.append(eng.debug_read("t").astype(np.int64)); es.append(eng.debug_read("eps"))
        assert not np.array_equal(ts[0], ts[1]) and not np.array_equal(es[0], es[1])
        t = np.concatenate(ts)
        assert t.min() == 0 and t.max() == c["N"] - 1
        p = stats.chisquare(np.bincount(t, minlength=c["N"])).pvalue
        e = np.concatenate(es).astype(np.float64)
        print(f"t: chi-square p {p:.3f} over {t.size}; eps: mean {e.mean():.4f}, std {e.std():.4f} over {e.size}")
        assert p > 1e-4
        _moments_ok(e, "eps")
        assert stats.kstest(e, "norm").pvalue > 1e-3, stats.kstest(e, "norm")
        obs = np.random.RandomState(0).standard_normal((B, c["obs_dim"])).astype(np.float32)
        x0 = np.random.RandomState(1).standard_normal((B, c["act_dim"])).astype(np.float32)
        zs = []
        for _ in range(calls):                                           # the tap holds the z of a call's last noisy step (t = 1)
            a = eng.sample(obs, x0)
            zs.append(eng.debug_read("z"))
            assert np.isfinite(a).all()
        assert not np.array_equal(zs[0], zs[1])                          # another call, another stream
        z = np.concatenate(zs).astype(np.float64)
        print(f"z: mean {z.mean():.4f}, std {z.std():.4f} over {z.size}")
        _moments_ok(z, "z")
        assert stats.kstest(z, "norm").pvalue > 1e-3, stats.kstest(z, "norm")
    finally:
        eng.close()


# ---- 6. an epoch in one call == the same steps one by one ------------------------------------------------------------------------------------
def test_epoch_equals_its_steps():
    c = dc.CASES["d"]
    order = np.random.RandomState(5).permutation(c["n"]).astype(np.int64)
    a, P = make_engine(c, seed=9)
    b, _ = make_engine(c, seed=9)
    try:
        la = np.concatenate([a.learn_epoch(order), a.learn_epoch(torch.as_tensor(order[::-1].copy(), device=DEV))])
        lb = [b.step(o[s:s + c["B"]]) for o in (order, order[::-1]) for s in range(0, c["n"], c["B"])]
        assert la.shape == (4,) and np.array_equal(la, np.array(lb, np.float32))
        assert a.step_count == b.step_count == 4
        for which in (a.PARAMS, a.EMA, a.EXP_AVG, a.EXP_AVG_SQ):
            assert np.array_equal(a.get(which), b.get(which))
        assert not np.array_equal(a.get(a.PARAMS), pack(a, P))           # (steps 1 .. 3 have lr > 0)
    finally:
        a.close(); b.close()


def test_engine_refusals():
    from offlinerlkit import _engine
    base = dict(obs_dim=5, act_dim=3, step_embed_dim=16, down_dims=[8, 16], batch_size=6)
    for over, msg in ((dict(n_runs=2), "one run per object"), (dict(precision=1), "precision 0"), (dict(kernel_size=4), "kernel_size must be odd"),
                      (dict(down_dims=[12, 16]), "multiple of n_groups"), (dict(step_embed_dim=15), "step_embed_dim"),
                      (dict(down_dims=[12, 16], n_groups=4), "multiple of 8")):
        with pytest.raises(RuntimeError, match=msg):
            _engine.Diffusion(_engine.default_diffusion_config(**dict(base, **over)))
    c = dc.CASES["b"]
    eng, _ = make_engine(c, total_steps=1)
    try:
        idx, t, eps = dc.make_steps(c, 1)[0]
        eng.step(idx, t, eps)
        with pytest.raises(RuntimeError, match="past the learning-rate table"):
            eng.step(idx, t, eps)
        with pytest.raises(RuntimeError, match="row index out of range"):
            eng.step(np.array([c["n"]], np.int64))
        with pytest.raises(RuntimeError, match="batch_size"):
            eng.step(np.zeros(c["B"] + 1, np.int64))
        assert eng.step_count == 1
    finally:
        eng.close()


# ---- 7. the policy class and the device rollout -------------------------------------------------------------------------------------------------
class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _policy(c, tmp, od=None, ad=None, data=None, **over):
    from offlinerlkit.policy import DiffusionBC
    from offlinerlkit.utils.diffusion_logger import Logger
    od, ad = od or c["obs_dim"], ad or c["act_dim"]
    cfg = _Cfg(act_dim=ad, obs_dim=od, num_epochs=3, num_diffusion_iters=c["N"], batch_size=c["B"], save_ckpt_freq=1, device=DEV, path=None,
               num_workers=1, spectral_norm=False, seed=3, **dc.net_kwargs(c))
    cfg.__dict__.update(over)
    torch.manual_seed(11)
    return DiffusionBC(cfg, data if data is not None else dc.make_data(c), Logger(str(tmp)))


def test_policy_trains_samples_and_checkpoints(tmp_path):
    c = dc.CASES["d"]
    pol = _policy(c, tmp_path)
    before = {k: v.clone() for k, v in pol.noise_pred_net.state_dict().items()}
    pol.train()
    after = pol.noise_pred_net.state_dict()
    moved = [k for k in before if not torch.equal(before[k], after[k])]
    assert len(moved) == len(before), set(before) - set(moved)        # every tensor trained (5 of 6 steps have lr > 0)
    for k, v in after.items():                                          # ... by its centre tap only
        if v.dim() == 3 and v.shape[2] > 1:
            keep = [i for i in range(v.shape[2]) if i != v.shape[2] // 2]
            assert torch.equal(v[:, :, keep], before[k][:, :, keep])
    assert (tmp_path / "checkpoint.pt").exists() and (tmp_path / "progress.csv").exists()
    obs = np.random.RandomState(2).standard_normal((5, c["obs_dim"])).astype(np.float32)
    noise = pol.sample_init_noise(5)
    assert noise.shape == (5, 1, c["act_dim"]) and noise.device.type == "cuda"
    pol2 = _policy(c, tmp_path / "second", num_epochs=3)
    pol.save_checkpoint(None)
    pol2.c.path = str(tmp_path)
    assert pol2.load_checkpoint(final=True)
    a_dev = pol.select_action_device(torch.as_tensor(obs, device=DEV), noise)
    a_host = pol2.select_action(obs, noise)                             # a second policy from models.pt: the same EMA weights, the same z stream
    assert isinstance(a_host, np.ndarray) and a_host.shape == (5, c["act_dim"]) and a_dev.device.type == "cuda"
    assert np.array_equal(a_dev.cpu().numpy(), a_host)
    assert pol2.select_action(obs[0], noise[:1]).shape == (c["act_dim"],)
    assert np.abs(a_host).max() <= 1.0 + 1e-6                            # the last step has no noise: x = the clipped x0


def test_rollout_device_with_frozen_noise_matches_the_host_rollout(tmp_path):
    import rcsl_rollout_ref as ref
    from test_gpu_rcsl_rollout import _rcsl_policy
    from test_gpu_training import AD, OD, make_dataset
    from offlinerlkit import _engine
    from offlinerlkit.buffer import ReplayBuffer
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.modules import EnsembleDynamicsModel
    from offlinerlkit.utils.logger import Logger
    from offlinerlkit.utils.scaler import StandardScaler
    from offlinerlkit.utils.termination_fns import TERM_ANT, termination_fn_ant
    torch.manual_seed(5)
    np.random.seed(5)
    ds = make_dataset(n_episodes=60)
    logger = Logger(str(tmp_path), {"consoleout_backup": "stdout", "dynamics_training_progress": "csv"})

    def dynamics():
        model = EnsembleDynamicsModel(OD, AD, [32, 32], num_ensemble=3, num_elites=2, weight_decays=[2.5e-5, 5e-5, 1e-4], device=DEV)
        d = EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), StandardScaler(), termination_fn_ant,
                             penalty_coef=0.5, uncertainty_mode="aleatoric")
        d.set_engine_options(seed=77)
        return d
    dyn_a = dynamics()
    data = ReplayBuffer(len(ds["rewards"]), (OD,), np.float32, AD, np.float32, device=DEV)
    data.load_dataset(ds)
    dyn_a.train(data.sample_all(), logger, max_epochs=2, max_epochs_since_update=2)
    dyn_b = dynamics()
    dyn_b.load(logger.model_dir)
    c = dc.CASES["d"]
    bc = (ds["observations"][:64].astype(np.float32), np.tanh(ds["actions"][:64]).astype(np.float32))
    pol_a = _policy(c, tmp_path / "a", od=OD, ad=AD, data=bc)
    pol_b = _policy(c, tmp_path / "b", od=OD, ad=AD, data=bc)
    assert pol_a.device_frozen_noise is True
    n_traj, L = 6, 4
    rng = np.random.RandomState(1)
    init = np.stack([rng.uniform(0.25, 0.95, n_traj), rng.uniform(-1.5, 1.5, n_traj)], 1).astype(np.float32)   # x0 around TERM_ANT's bounds
    rp = _rcsl_policy(dyn_a, pol_a, OD, AD)
    torch.manual_seed(123)
    host, hinfo = rp.rollout(init, L)
    rp.dynamics, rp.rollout_policy = dyn_b, pol_b
    store = _engine.TrajStore(OD, AD, n_traj, n_traj * L)
    seen = []
    live_index = store.live_index
    store.live_index = lambda: seen.append(live_index().cpu().numpy()) or torch.as_tensor(seen[-1], device=DEV)
    torch.manual_seed(123)
    roll, dinfo = rp.rollout_device(init, L, store=store)
    term = host["terminals"].ravel()
    per_step, row = [], 0
    while row < len(term):
        n = n_traj if not per_step else int((~term[row - len(per_step[-1]):row]).sum())
        per_step.append(host["traj_idxs"][row:row + n]); row += n
    print(f"host rollout: {len(term)} transitions, live per step {[len(p) for p in per_step]}")
    assert len(term) < n_traj * L and len(per_step) > 1                  # some trajectories end early
    assert len(seen) == len(per_step) and all(np.array_equal(s, p) for s, p in zip(seen, per_step))
    got = roll.to_host()
    for k in ref.KEYS:
        assert got[k].dtype == host[k].dtype and got[k].shape == host[k].shape, k
        assert np.array_equal(ref.bits(got[k]), ref.bits(host[k])), k
    assert dinfo["num_transitions"] == hinfo["num_transitions"]
    assert np.array_equal(ref.bits(dinfo["returns"]), ref.bits(hinfo["returns"]))

#!/usr/bin/env python3
"""RCSL epoch throughput at run_rcsl.py's shape on hopper (obs 11, act 3, MLP [200] x 4 on [obs | rtg], batch 256, lr 1e-3): one
``RcslPolicy.learn_epoch`` (orl_learn_epoch: ordered gather, forward, masked MSE, backward, Adam per step, one host sync per epoch) at 1
and at 8 runs per engine, against a stock-torch restatement of the same epoch on the same GPU (torch.randperm order, index_select from
device-resident arrays, nn.Linear / ReLU forward, autograd, torch.optim.Adam, one ``.item()`` per batch like the reference's ``learn``;
R runs = R such models trained one after the other).  One invocation, alternating: a warm-up epoch of each, then ``--blocks`` timed
epochs of each, timed with a host clock around work that ends in a device synchronise.  A synthetic dataset of ``--rows`` rows (default
100 000 = 391 steps, the last batch partial).  The figure is run-steps per second.  Prints one JSON object; --out writes it too.  Needs a GPU.
``--gauss``: the same measurement of ``RcslGaussianPolicy`` at run_rcsl_gauss.py's shape (MLP [1024] x 4 down to an act_dim-wide latent, the
DiagGaussian head with a clamped state-conditioned sigma, Gaussian NLL; k_rcslg_head in place of the MSE launch).
``--autoreg``: ``AutoregressivePolicy`` at run_regress.py's shape on hopper ([200] x 4 on 11 + 3 + 3 = 17 inputs, batch 256 = 768 expanded
rows per step, LeakyReLU on the tiled GEMM, k_autoreg_head) against the torch ``fit`` of an unbound policy object (plain nn.Linear /
nn.LeakyReLU, autograd, torch.optim.Adam); and, in the same run, ``select_action`` on 256 rows (orl_autoreg_sample: 3 forward-only passes
with k_autoreg_draw between them, the normals from torch.randn) against the reference's sequential torch loop over the same rows
(``sampling``: calls per second, alternating blocks of ``--sample-calls`` calls).
``--rollout``: the rollout stage of run_mbrcsl.py at its shape on hopper -- ``RcslPolicy.rollout`` (host bookkeeping, arrays through the host
every model step) against ``RcslPolicy.rollout_device`` (``TrajStore``: orl_traj_*) on the same GPU: an ``EnsembleDynamics`` of 7 members /
5 elites, [200] x 4, an ``AutoregressivePolicy`` [200] x 4, ``--trajectories`` (256) trajectories of ``--horizon`` (1000) steps, a termination
function that never fires so the length is fixed, freshly initialised nets (the work per step does not depend on the weights).  A warm-up
rollout of each, then ``--blocks`` timed rollouts of each, alternating; the figure is transitions per second.  Then, once, the wall time
of the device path's pieces over one more rollout (action sampling, dynamics step, store append; each ends in a host synchronisation).
A third contestant runs in the same alternation: ``rollout_device(fused=True)`` (orl_mbrcsl_rollout: every launch of every step on one
stream, step t sized by the survivor count of step t - 1 - lag) at the default ``lag`` = 2, with the HIP-event time of its loop next to
the wall time of the call; then one rollout each at ``lag`` 0, 1, 2 and 4.
Writes profiles/rcsl_rollout_fused_throughput.json unless --out names another file.
``--diffusion``: ``DiffusionBC`` at the default shape on hopper (ConditionalUnet1D [256, 512, 1024], embedding 256, N = 10, batch 256), three
figures from one run: (1) one training epoch over ``--rows`` rows (orl_diffusion_learn_epoch) against autograd + torch.optim.Adam on the
project's own ``ConditionalUnet1D`` on the same GPU (steps per second); (2) ``select_action`` on 256 rows (orl_diffusion_sample: 10
forward-only passes) against the same DDPM loop in torch on that module (calls per second); (3) ``RcslPolicy.rollout_device`` with the
frozen noise in HBM against the host ``rollout()`` (transitions per second; ``--trajectories`` x ``--horizon``).  Writes
profiles/diffusion_throughput.json unless --out names another file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "offlinerl-kit_amd"))
from offlinerlkit import _engine  # noqa: E402
from offlinerlkit.modules import DiagGaussian, RcslGaussianModule, RcslModule  # noqa: E402
from offlinerlkit.nets import MLP  # noqa: E402
from offlinerlkit.policy import AutoregressivePolicy, RcslGaussianPolicy, RcslPolicy  # noqa: E402
from offlinerlkit.policy.rcsl import epoch_order  # noqa: E402

DEV = "cuda:0"
OD, AD, HID, B, LR = 11, 3, [200, 200, 200, 200], 256, 1e-3
HID_GAUSS = [1024, 1024, 1024, 1024]


def dataset(rows):
    rng = np.random.default_rng(0)
    return dict(observations=rng.normal(size=(rows, OD)).astype(np.float32), actions=rng.uniform(-1, 1, size=(rows, AD)).astype(np.float32),
                rtgs=rng.uniform(0, 3200, size=(rows, 1)).astype(np.float32))


def engine_epoch(pol, buf, rows, runs):
    order = epoch_order(rows, B, runs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pol.learn_epoch(buf, order, B)
    torch.cuda.synchronize()
    return (order.shape[1] // B) * runs / (time.perf_counter() - t0)


def torch_loss(net, x, act):
    if isinstance(net, AutoregressivePolicy):
        return net.fit(x[:, :OD], act)
    if isinstance(net, RcslGaussianModule):
        mu, logvar = net.dist_net.get_dist_params(net.backbone(x))
        return (torch.pow(mu - act, 2) * torch.exp(-logvar)).mean() + logvar.mean()
    return torch.pow(net(x) - act, 2).mean()


def torch_epoch(models, data, rows):
    steps = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for net, opt in models:
        perm = torch.randperm(rows, device=DEV)
        for s in range(0, rows, B):
            idx = perm[s:s + B]
            x = torch.cat([data["observations"].index_select(0, idx), data["rtgs"].index_select(0, idx)], dim=-1)
            loss = torch_loss(net, x, data["actions"].index_select(0, idx))
            opt.zero_grad()
            loss.backward()
            opt.step()
            loss.item()
            steps += 1
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def make_module(gauss):
    if gauss:
        return RcslGaussianModule(MLP(input_dim=OD + 1, hidden_dims=HID_GAUSS, output_dim=AD),
                                  DiagGaussian(AD, AD, unbounded=True, conditioned_sigma=True), DEV)
    return RcslModule(MLP(input_dim=OD + 1, hidden_dims=HID, output_dim=AD), DEV)


def torch_sample(pol, obs):
    """AutoregressivePolicy.forward of the reference for a batch of rows: act_dim sequential passes, one Normal.sample each"""
    n, A = obs.shape[0], pol.act_dim
    with torch.no_grad():
        act = torch.zeros((n, A), device=obs.device)
        eye = torch.eye(A, device=obs.device)
        for i in range(A):
            x = torch.cat([obs, act, eye[i][None, :].repeat(n, 1)], dim=1)
            for layer in pol.model:
                x = layer(x)
            mean, logstd = torch.chunk(x, 2, dim=-1)
            nxt = torch.distributions.Normal(mean, logstd.exp()).sample()
            act = torch.cat([act[:, :i], nxt, act[:, i + 1:]], dim=1)
        return act.cpu().numpy()


def measure_sampling(pol, ref, obs, blocks, calls):
    obs_t = torch.as_tensor(obs, device=DEV)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        torch.cuda.synchronize()
        return calls / (time.perf_counter() - t0)
    eng_f, ref_f = (lambda: pol.select_action(obs)), (lambda: torch_sample(ref, obs_t))
    timed(eng_f); timed(ref_f)
    eng, tor = [], []
    for _ in range(blocks):
        eng.append(timed(eng_f)); tor.append(timed(ref_f))
    return dict(rows=int(obs.shape[0]), calls_per_block=calls, engine_calls_per_s=eng, torch_calls_per_s=tor, engine_median=float(np.median(eng)),
                torch_median=float(np.median(tor)), speedup=float(np.median(eng) / np.median(tor)))


def measure(ds, rows, runs, blocks, gauss=False, autoreg=False, sample_calls=0):
    torch.manual_seed(1)
    if autoreg:
        pol = AutoregressivePolicy(OD, AD, HID, LR, DEV)
    else:
        mod = make_module(gauss)
        pol = (RcslGaussianPolicy if gauss else RcslPolicy)(None, None, mod, torch.optim.Adam(mod.parameters(), lr=LR), DEV)
    pol.set_engine_options(n_runs=runs, seed=3)
    buf = _engine.DeviceBuffer(OD, AD, 0)
    buf.load(ds["observations"], ds["actions"], ds["observations"], ds["rtgs"].reshape(rows), np.zeros(rows, np.float32))
    models = []
    for _ in range(runs):
        if autoreg:
            net = AutoregressivePolicy(OD, AD, HID, LR, DEV)      # (never bound to an engine: plain torch modules)
            models.append((net, net.rcsl_optim))
            continue
        net = make_module(True) if gauss else MLP(input_dim=OD + 1, hidden_dims=HID, output_dim=AD).to(DEV)
        models.append((net, torch.optim.Adam(net.parameters(), lr=LR)))
    data = {k: torch.as_tensor(v, device=DEV) for k, v in ds.items()}
    engine_epoch(pol, buf, rows, runs); torch_epoch(models, data, rows)          # warm-up: graph capture / allocator
    eng, ref = [], []
    for _ in range(blocks):
        eng.append(engine_epoch(pol, buf, rows, runs))
        ref.append(torch_epoch(models, data, rows))
    out = dict(runs=runs, engine_run_steps_per_s=eng, torch_run_steps_per_s=ref, engine_median=float(np.median(eng)),
               torch_median=float(np.median(ref)), speedup=float(np.median(eng) / np.median(ref)))
    if autoreg and sample_calls > 0:
        out["sampling"] = measure_sampling(pol, models[0][0], ds["observations"][:256], blocks, sample_calls)
    return out


def measure_rollout(n_traj, horizon, blocks):
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.modules import EnsembleDynamicsModel
    from offlinerlkit.utils.scaler import StandardScaler
    from offlinerlkit.utils.termination_fns import termination_fn_default
    torch.manual_seed(1)
    model = EnsembleDynamicsModel(OD, AD, HID, num_ensemble=7, num_elites=5, weight_decays=[2.5e-5, 5e-5, 7.5e-5, 7.5e-5, 1e-4], device=DEV)
    scaler = StandardScaler(np.zeros((1, OD + AD), np.float32), np.ones((1, OD + AD), np.float32))
    dyn = EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), scaler, termination_fn_default)
    dyn.set_engine_options(seed=3)
    ar = AutoregressivePolicy(OD, AD, HID, LR, DEV)
    mod = make_module(False)
    pol = RcslPolicy(dyn, ar, mod, torch.optim.Adam(mod.parameters(), lr=LR), DEV)
    init = np.random.default_rng(0).normal(size=(n_traj, OD)).astype(np.float32)
    store = _engine.TrajStore(OD, AD, n_traj, n_traj * horizon, 0)

    def host():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, info = pol.rollout(init, horizon)
        torch.cuda.synchronize()
        return info["num_transitions"] / (time.perf_counter() - t0)

    def device():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, info = pol.rollout_device(init, horizon, store=store)
        torch.cuda.synchronize()
        return info["num_transitions"] / (time.perf_counter() - t0)

    def fused(lag=2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, info = pol.rollout_device(init, horizon, store=store, fused=True, lag=lag)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return info["num_transitions"] / wall, dict(lag=lag, transitions_per_s=info["num_transitions"] / wall, wall_ms=1e3 * wall,
                                                    loop_event_ms=float(info["loop_ms"]), steps_enqueued=int(info["steps_enqueued"]))
    host(); device(); fused()                          # warm-up: engine binding, allocator
    h, d, f, f_info = [], [], [], []
    for _ in range(blocks):
        h.append(host()); d.append(device())
        rate, info = fused()
        f.append(rate); f_info.append(info)
    per_lag = [fused(lag)[1] for lag in (0, 1, 2, 4)]
    # where the device path's time goes: the same loop with a clock around each piece (every piece ends in a host synchronisation)
    parts = dict(select_action_device=0.0, step_device=0.0, append_step=0.0)
    obs = torch.as_tensor(init, device=DEV)
    store.reset(n_traj)
    t_all = time.perf_counter()
    with torch.no_grad():
        for _ in range(horizon):
            t0 = time.perf_counter()
            act = ar.select_action_device(obs).contiguous()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            nxt, rew, _ = dyn.step_device(obs, act)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            alive = torch.empty_like(nxt)
            n_alive = store.append_step(dyn.term_kind, obs, act, nxt.contiguous(), rew.contiguous(), alive)
            t3 = time.perf_counter()
            parts["select_action_device"] += t1 - t0; parts["step_device"] += t2 - t1; parts["append_step"] += t3 - t2
            obs = alive[:n_alive]
    total = time.perf_counter() - t_all
    rows, rew_sum, _ = store.finish()
    return dict(trajectories=n_traj, horizon=horizon, transitions=rows, host_transitions_per_s=h, device_transitions_per_s=d,
                host_median=float(np.median(h)), device_median=float(np.median(d)), speedup=float(np.median(d) / np.median(h)),
                fused_transitions_per_s=f, fused_median=float(np.median(f)), fused_over_device=float(np.median(f) / np.median(d)),
                fused_ranges_disjoint=bool(min(f) > max(d)), fused_rollouts=f_info, fused_per_lag=per_lag,
                device_ms_per_step={k: 1e3 * v / horizon for k, v in parts.items()}, device_ms_per_step_total=1e3 * total / horizon,
                rewards_finite=bool(np.isfinite(rew_sum)))


def measure_diffusion(rows, blocks, sample_calls, n_traj, horizon):
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.modules import EnsembleDynamicsModel
    from offlinerlkit.nets import ConditionalUnet1D
    from offlinerlkit.policy import DiffusionBC
    from offlinerlkit.utils.diffusion_logger import Logger
    from offlinerlkit.utils.scaler import StandardScaler
    from offlinerlkit.utils.termination_fns import termination_fn_default

    class Cfg:
        act_dim, obs_dim, num_epochs, num_diffusion_iters, batch_size, save_ckpt_freq = AD, OD, 1000, 10, B, 10 ** 9
        device, path, num_workers, spectral_norm = DEV, None, 1, False
    ds = dataset(rows)
    torch.manual_seed(0)
    bc = DiffusionBC(Cfg(), (ds["observations"], ds["actions"]), Logger(None))
    eng = bc._attach()
    net = ConditionalUnet1D(AD, OD).to(DEV)
    net.load_state_dict(bc.noise_pred_net.state_dict())
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    obs_d, act_d = torch.as_tensor(ds["observations"], device=DEV), torch.as_tensor(ds["actions"], device=DEV)
    acp = torch.as_tensor(bc.alphas_cumprod, device=DEV)
    steps = -(-rows // B)

    def engine_epoch():
        order = torch.randperm(rows, device=DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = eng.learn_epoch(order)
        return steps / (time.perf_counter() - t0), float(losses[-1])

    def torch_epoch():
        order = torch.randperm(rows, device=DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(0, rows, B):
            idx = order[s:s + B]
            a = act_d[idx].unsqueeze(1)
            noise = torch.randn_like(a)
            t = torch.randint(0, 10, (len(idx),), device=DEV)
            xt = acp[t].sqrt().reshape(-1, 1, 1) * a + (1 - acp[t]).sqrt().reshape(-1, 1, 1) * noise
            loss = torch.nn.functional.mse_loss(net(xt, t, global_cond=obs_d[idx]), noise)
            opt.zero_grad()
            loss.backward()
            opt.step()
            last = loss.item()                          # one read per batch, like the reference's record_mean(loss.item())
        torch.cuda.synchronize()
        return steps / (time.perf_counter() - t0), last
    engine_epoch(); torch_epoch()
    e, r = [], []
    for _ in range(blocks):
        e.append(engine_epoch()); r.append(torch_epoch())
    train = dict(rows=rows, steps_per_epoch=steps, engine_steps_per_s=[x[0] for x in e], torch_steps_per_s=[x[0] for x in r],
                 engine_median=float(np.median([x[0] for x in e])), torch_median=float(np.median([x[0] for x in r])),
                 last_losses=dict(engine=e[-1][1], torch=r[-1][1]))
    train["speedup"] = train["engine_median"] / train["torch_median"]
    # (2) select_action on 256 rows: the engine's EMA weights are the initial ones of `bc`; torch runs the same loop on a copy of them
    ema = ConditionalUnet1D(AD, OD).to(DEV)
    ema.load_state_dict(bc.noise_pred_net.state_dict())
    coef = torch.as_tensor(bc.ddpm_coef, device=DEV)
    o256 = obs_d[:256].contiguous()

    def engine_sample():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(sample_calls):
            bc.select_action_device(o256, None)
        torch.cuda.synchronize()
        return sample_calls / (time.perf_counter() - t0)

    def torch_sample():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for _ in range(sample_calls):
                x = torch.randn((256, 1, AD), device=DEV)
                for t in range(9, -1, -1):
                    e_ = ema(x, t, global_cond=o256)
                    x0 = ((x - coef[t, 1] * e_) / coef[t, 0]).clamp(-1, 1)
                    x = coef[t, 2] * x0 + coef[t, 3] * x
                    if t > 0:
                        x = x + coef[t, 4] * torch.randn_like(x)
                x.cpu()
        return sample_calls / (time.perf_counter() - t0)
    engine_sample(); torch_sample()
    se, st = [], []
    for _ in range(blocks):
        se.append(engine_sample()); st.append(torch_sample())
    sampling = dict(rows=256, engine_calls_per_s=se, torch_calls_per_s=st, engine_median=float(np.median(se)), torch_median=float(np.median(st)),
                    speedup=float(np.median(se) / np.median(st)))
    # (3) the rollout stage with the diffusion behaviour policy
    torch.manual_seed(1)
    model = EnsembleDynamicsModel(OD, AD, HID, num_ensemble=7, num_elites=5, weight_decays=[2.5e-5, 5e-5, 7.5e-5, 7.5e-5, 1e-4], device=DEV)
    scaler = StandardScaler(np.zeros((1, OD + AD), np.float32), np.ones((1, OD + AD), np.float32))
    dyn = EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), scaler, termination_fn_default)
    dyn.set_engine_options(seed=3)
    mod = make_module(False)
    pol = RcslPolicy(dyn, bc, mod, torch.optim.Adam(mod.parameters(), lr=LR), DEV)
    init = np.random.default_rng(0).normal(size=(n_traj, OD)).astype(np.float32)
    store = _engine.TrajStore(OD, AD, n_traj, n_traj * horizon, 0)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, info = fn()
        torch.cuda.synchronize()
        return info["num_transitions"] / (time.perf_counter() - t0)
    host = lambda: timed(lambda: pol.rollout(init, horizon))
    device = lambda: timed(lambda: pol.rollout_device(init, horizon, store=store))
    h, dv = [], []
    for i in range(blocks + 1):                          # the first pair is the warm-up
        a, b = host(), device()
        if i:
            h.append(a); dv.append(b)
    rollout = dict(trajectories=n_traj, horizon=horizon, host_transitions_per_s=h, device_transitions_per_s=dv, host_median=float(np.median(h)),
                   device_median=float(np.median(dv)), speedup=float(np.median(dv) / np.median(h)))
    return dict(training_epoch=train, select_action=sampling, rollout=rollout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--runs", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--gauss", action="store_true", help="RcslGaussianPolicy at run_rcsl_gauss.py's shape ([1024] x 4)")
    ap.add_argument("--autoreg", action="store_true", help="AutoregressivePolicy at run_regress.py's shape ([200] x 4, 768 expanded rows), and select_action on 256 rows")
    ap.add_argument("--sample-calls", type=int, default=50)
    ap.add_argument("--rollout", action="store_true", help="RcslPolicy.rollout against rollout_device at run_mbrcsl.py's shape on hopper")
    ap.add_argument("--trajectories", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--diffusion", action="store_true", help="DiffusionBC at the default shape: a training epoch, select_action on 256 rows, the rollout")
    a = ap.parse_args()
    if a.diffusion:
        res = dict(policy="DiffusionBC", shape=dict(obs_dim=OD, act_dim=AD, down_dims=[256, 512, 1024], step_embed_dim=256, kernel_size=5,
                                                    n_groups=8, num_diffusion_iters=10, batch=B),
                   device=torch.cuda.get_device_name(0), blocks=a.blocks,
                   result=measure_diffusion(a.rows, a.blocks, a.sample_calls, a.trajectories, a.horizon))
        print(json.dumps(res))
        with open(a.out or os.path.join(ROOT, "profiles", "diffusion_throughput.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    if a.rollout:
        res = dict(stage="RcslPolicy.rollout vs rollout_device vs rollout_device(fused=True)", shape=dict(obs_dim=OD, act_dim=AD, dynamics_hidden=HID, ensemble=7, elites=5,
                                                                          behaviour_hidden=HID, termination="none"),
                   device=torch.cuda.get_device_name(0), result=measure_rollout(a.trajectories, a.horizon, a.blocks))
        print(json.dumps(res))
        with open(a.out or os.path.join(ROOT, "profiles", "rcsl_rollout_fused_throughput.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    ds = dataset(a.rows)
    res = dict(policy="AutoregressivePolicy" if a.autoreg else "RcslGaussianPolicy" if a.gauss else "RcslPolicy", precision=int(os.environ.get("ORL_PRECISION", "0")),
               shape=dict(obs_dim=OD, act_dim=AD, hidden=HID_GAUSS if a.gauss else HID, batch=B, rows=a.rows, steps_per_epoch=-(-a.rows // B)),
               device=torch.cuda.get_device_name(0), results=[measure(ds, a.rows, r, a.blocks, a.gauss, a.autoreg, a.sample_calls) for r in a.runs])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

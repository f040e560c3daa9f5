#!/usr/bin/env python3
"""Model-based training-loop throughput at the halfcheetah shape of run_mopo.py / run_combo.py (obs 17, act 6, dynamics [200] x 4 with
7 members, policy [256, 256] (COMBO [256, 256, 256]), batch 256, real_ratio 0.05 (COMBO 0.5), rollouts (1000, 50 000, 5), model buffer
1.25 M rows, a synthetic 1 M-row dataset, the halfcheetah termination test): MBPolicyTrainer's host loop (fused=False) against the fused
loop (fused=True), in ONE invocation and alternating -- a warm-up block of each, then three timed blocks each of 2 000 training steps
including their two rollouts, timed with a host clock around work that ends in a device synchronise.  Also the rollout alone (ms per
50 000 x 5 rollout, both paths).  Everything is built from seeds (an untrained dynamics ensemble with a unit scaler: the arithmetic per
row is that of a trained one).  Prints one JSON object; --out writes it too.  Needs a GPU.

--runs R measures, instead, R independent seeds in the same invocation and alternating the same way: ONE R-run policy with per-run model
rings (a list of R model buffers: every run rolls its own actor through its own run of an R-run dynamics into its own ring) against the
baseline of R single-run fused trainings run one after the other, each with its own policy, dynamics and ring.  The figure is aggregate
run-steps per second: R x block steps / seconds of the block, rollouts included.

--rambo measures, instead, RAMBO's adversarial model update at run_rambo.py's shape (dynamics [200] x 4, 7 members, 5 elites, policy
[256, 256], 256 rollout + 256 dataset rows per step, adv_rollout_length 5, adv_weight 3e-4, 1000 steps per update):
``RAMBOPolicy.update_dynamics`` on the engine against a stock-torch restatement of the same update (the reference's
``dynamics_step_and_forward`` with torch autograd and torch.optim.Adam on the same GPU, same buffer draws, actor and critics) and against
``RAMBOPolicy.update_dynamics_device`` (the whole update as one device loop, ``orl_rambo_update_dynamics``), a warm-up of each and then
alternating timed updates, each window ending in a device synchronise.  The figure is model-update steps per second (means and medians
over the windows; ``--blocks 5`` for medians of five).

--mobile measures, instead, ``MOBILEPolicy.learn`` in the host loop at run_mobile.py's shape (policy [256, 256], dynamics [200] x 4, 7
members, 5 elites, 10 samples: 12 800 penalty rows per step, batch 256 with 12 real rows, penalty_coef 1.5, deterministic backup) against
a stock-torch restatement of the same step (mobile.py:130-196 with torch autograd and torch.optim.Adam on the same GPU, same batches), a
warm-up of each and then alternating timed blocks; the figure is gradient steps per second.  It also prints the HIP-event split of one
block into the penalty pass (the ``lcb`` launches of orl_profile_query) and the rest of the step.  The third contestant is
``MOBILEDevicePolicy.learn_n``: the same steps as one device loop (``orl_mobile_learn_n``; batches drawn on the device from the same
dataset and the same model rows held in an HBM ring), one call per block, with the HIP-event time of the loop next to the wall time
(``--blocks 5`` for medians of five)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "offlinerl-kit_amd"))
from offlinerlkit.buffer import ReplayBuffer  # noqa: E402
from offlinerlkit.dynamics import EnsembleDynamics  # noqa: E402
from offlinerlkit.modules import ActorProb, Critic, EnsembleDynamicsModel, TanhDiagGaussian  # noqa: E402
from offlinerlkit.nets import MLP  # noqa: E402
from offlinerlkit.policy import COMBOPolicy, MOBILEDevicePolicy, MOBILEPolicy, MOPOPolicy, RAMBOPolicy  # noqa: E402
from offlinerlkit.policy_trainer import MBPolicyTrainer  # noqa: E402
from offlinerlkit.utils.scaler import StandardScaler  # noqa: E402
from offlinerlkit.utils.termination_fns import termination_fn_halfcheetah  # noqa: E402

DEV = "cuda:0"
OD, AD, DYN_HID, K, E, B = 17, 6, [200, 200, 200, 200], 7, 5, 256
DECAYS = [2.5e-5, 5e-5, 7.5e-5, 7.5e-5, 1e-4]
ROLLOUT = (1000, 50_000, 5)
MODEL_ROWS, DATA_ROWS, BLOCK = 1_250_000, 1_000_000, 2_000


class Space:
    low, high, shape = -np.ones(AD, np.float32), np.ones(AD, np.float32), (AD,)


class NullLogger:
    def log(self, *a, **k):
        pass

    def logkv(self, *a, **k):
        pass

    logkv_mean = logkv


def dataset(rows):
    rng = np.random.default_rng(0)
    obs = rng.normal(size=(rows, OD)).astype(np.float32)
    return dict(observations=obs, actions=rng.uniform(-1, 1, size=(rows, AD)).astype(np.float32),
                next_observations=(obs + 0.1 * rng.normal(size=(rows, OD))).astype(np.float32),
                rewards=rng.normal(size=rows).astype(np.float32), terminals=np.zeros(rows, np.float32))


def make_policy(algo, n_runs=1, seed=0):
    torch.manual_seed(1 + seed)
    model = EnsembleDynamicsModel(OD, AD, DYN_HID, num_ensemble=K, num_elites=E, weight_decays=DECAYS, device=DEV)
    scaler = StandardScaler(np.zeros((1, OD + AD), np.float32), np.ones((1, OD + AD), np.float32))
    dyn = EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), scaler, termination_fn_halfcheetah,
                           penalty_coef=2.5 if algo == "mopo" else 0.0, uncertainty_mode="aleatoric")
    dyn.set_engine_options(n_runs=n_runs, seed=7 + seed)
    hid = [256, 256] if algo == "mopo" else [256, 256, 256]
    adam = lambda m, lr: torch.optim.Adam(m.parameters(), lr=lr)
    actor = ActorProb(MLP(OD, hid), TanhDiagGaussian(hid[-1], AD, unbounded=True, conditioned_sigma=True), DEV)
    c1, c2 = Critic(MLP(OD + AD, hid), DEV), Critic(MLP(OD + AD, hid), DEV)
    log_alpha = torch.zeros(1, requires_grad=True, device=DEV)
    alpha = (-float(AD), log_alpha, torch.optim.Adam([log_alpha], lr=1e-4))
    if algo == "mopo":
        pol = MOPOPolicy(dyn, actor, c1, c2, adam(actor, 1e-4), adam(c1, 3e-4), adam(c2, 3e-4), tau=0.005, gamma=0.99, alpha=alpha)
    else:
        pol = COMBOPolicy(dyn, actor, c1, c2, adam(actor, 1e-4), adam(c1, 3e-4), adam(c2, 3e-4), Space(), tau=0.005, gamma=0.99, alpha=alpha,
                          cql_weight=5.0, temperature=1.0, max_q_backup=False, deterministic_backup=True, with_lagrange=False,
                          num_repeart_actions=10, uniform_rollout=False, rho_s="mix")
    pol.set_engine_options(n_runs=n_runs, seed=3 + seed)
    return pol


def measure_runs(algo, ds, blocks, block_steps, runs):
    """per-run rings at ``runs`` runs against ``runs`` single-run fused trainings one after the other"""
    real_ratio = 0.05 if algo == "mopo" else 0.5
    real = ReplayBuffer(len(ds["rewards"]), (OD,), np.float32, AD, np.float32, device=DEV)
    real.load_dataset(ds)
    fake = lambda: ReplayBuffer(MODEL_ROWS, (OD,), np.float32, AD, np.float32, device=DEV)
    trainer = lambda pol, fk: MBPolicyTrainer(pol, None, real, fk, NullLogger(), ROLLOUT, epoch=1, step_per_epoch=block_steps, batch_size=B,
                                              real_ratio=real_ratio, fused=True)
    pol = make_policy(algo, n_runs=runs)
    pol.train()
    batched = trainer(pol, [fake() for _ in range(runs)])
    singles = []
    for r in range(runs):
        p1 = make_policy(algo, seed=100 + r)
        p1.train()
        singles.append(trainer(p1, fake()))
    t_now = {"per_run_rings": 0, "sequential": 0}

    def block(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "per_run_rings":
            t_now[name] = batched._train_mb_epoch(1, t_now[name])
        else:
            for tr in singles:
                end = tr._train_mb_epoch(1, t_now[name])
            t_now[name] = end
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    names = ("sequential", "per_run_rings")
    np.random.seed(0)
    torch.manual_seed(0)
    warm = {name: block(name) for name in names}
    secs = {name: [] for name in names}
    for _ in range(blocks):
        for name in names:
            secs[name].append(block(name))
    rsps = {name: [runs * block_steps / s for s in v] for name, v in secs.items()}
    base_spread = max(rsps["sequential"]) - min(rsps["sequential"])
    gain = float(np.mean(rsps["per_run_rings"]) - np.mean(rsps["sequential"]))
    return dict(algo=algo, runs=runs, real_ratio=real_ratio, block_steps=block_steps,
                rollouts_per_block=len([t for t in range(block_steps) if t % ROLLOUT[0] == 0]), warmup_block_seconds=warm, block_seconds=secs,
                run_steps_per_s=rsps, run_steps_per_s_mean={k: float(np.mean(v)) for k, v in rsps.items()},
                sequential_spread_run_steps_per_s=base_spread, per_run_rings_minus_sequential_run_steps_per_s=gain,
                clears_bar=bool(gain > base_spread), speedup=float(np.mean(rsps["per_run_rings"]) / np.mean(rsps["sequential"])),
                model_rows=dict(per_run_rings=[b._size for b in batched.fake_buffer], sequential=[tr.fake_buffer._size for tr in singles]))


def measure(algo, ds, blocks, block_steps, profile_only=False):
    real_ratio = 0.05 if algo == "mopo" else 0.5
    real = ReplayBuffer(len(ds["rewards"]), (OD,), np.float32, AD, np.float32, device=DEV)
    real.load_dataset(ds)
    pol = make_policy(algo)
    pol.train()
    trainers, t_now = {}, {}
    for name in ("host", "fused"):
        fake = ReplayBuffer(MODEL_ROWS, (OD,), np.float32, AD, np.float32, device=DEV)
        trainers[name] = MBPolicyTrainer(pol, None, real, fake, NullLogger(), ROLLOUT, epoch=1, step_per_epoch=block_steps, batch_size=B,
                                         real_ratio=real_ratio, fused=(name == "fused"))
        t_now[name] = 0

    def block(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t_now[name] = trainers[name]._train_mb_epoch(1, t_now[name])
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    if profile_only:
        block("fused")
        return dict(algo=algo, fused_block_seconds=block("fused"))
    np.random.seed(0)
    torch.manual_seed(0)
    warm = {name: block(name) for name in ("host", "fused")}
    secs = {"host": [], "fused": []}
    for _ in range(blocks):
        for name in ("host", "fused"):
            secs[name].append(block(name))
    sps = {name: [block_steps / s for s in v] for name, v in secs.items()}

    def rollout_ms(name, reps=3):
        tr, out = trainers[name], []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr._rollout_fused() if name == "fused" else tr._rollout()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return out
    roll = {name: rollout_ms(name) for name in ("host", "fused")}
    host_spread = max(sps["host"]) - min(sps["host"])
    gain = float(np.mean(sps["fused"]) - np.mean(sps["host"]))
    return dict(algo=algo, real_ratio=real_ratio, block_steps=block_steps, rollouts_per_block=len([t for t in range(block_steps) if t % ROLLOUT[0] == 0]),
                warmup_block_seconds=warm, block_seconds=secs, steps_per_s=sps,
                steps_per_s_mean={k: float(np.mean(v)) for k, v in sps.items()}, host_spread_steps_per_s=host_spread,
                fused_minus_host_steps_per_s=gain, clears_bar=bool(gain > host_spread),
                speedup=float(np.mean(sps["fused"]) / np.mean(sps["host"])),
                rollout_ms=roll, rollout_ms_mean={k: float(np.mean(v)) for k, v in roll.items()},
                model_rows={name: trainers[name].fake_buffer._size for name in trainers})


def torch_update_dynamics(pol, model, optim, mu, std, real, steps, rows, length, adv_weight, gamma):
    """rambo.py:95-207 in stock torch on the GPU: the loop of ``update_dynamics`` around an autograd ``dynamics_step_and_forward``"""
    done, info = 0, {}
    elites = model.elites.data
    while done < steps:
        obs = real.sample(rows)["observations"]
        for _ in range(length):
            with torch.no_grad():
                act, _ = pol.actforward(obs, False)
            b = real.sample(rows)
            x = (torch.cat([obs, act], -1) - mu) / std
            diff_mean, logvar = model(x)
            mean = torch.cat([diff_mean[..., :-1] + obs, diff_mean[..., -1:]], -1)
            dist = torch.distributions.Normal(mean, torch.sqrt(torch.exp(logvar)))
            ens = dist.sample()
            idx = torch.as_tensor(model.random_elite_idxs(rows), device=obs.device)
            sample = ens[idx, torch.arange(rows, device=obs.device)]
            nxt, rew = sample[..., :-1], sample[..., -1:]
            term = torch.as_tensor(termination_fn_halfcheetah(obs.cpu().numpy(), act.cpu().numpy(), nxt.cpu().numpy()), device=obs.device)
            lp = dist.log_prob(sample).sum(-1, keepdim=True)[elites]
            log_prob = (lp.double().exp() * (1 / len(elites))).sum(0).log().float()
            with torch.no_grad():
                na, _ = pol.actforward(nxt, True)
                next_q = torch.minimum(pol.critic1(nxt, na), pol.critic2(nxt, na))
                value = rew + (1 - term.float()) * gamma * next_q
                adv = value - torch.minimum(pol.critic1(obs, act), pol.critic2(obs, act))
                adv = (adv - adv.mean()) / (adv.std() + 1e-6)
            adv_loss = (log_prob * adv).mean()
            sx = (torch.cat([b["observations"], b["actions"]], -1) - mu) / std
            target = torch.cat([b["next_observations"] - b["observations"], b["rewards"]], -1)
            sm, slv = model(sx)
            sl = (torch.pow(sm - target, 2) * torch.exp(-slv)).mean(dim=(1, 2)).sum() + slv.mean(dim=(1, 2)).sum()
            sl = sl + model.get_decay_loss() + 0.001 * model.max_logvar.sum() - 0.001 * model.min_logvar.sum()
            loss = adv_weight * adv_loss + sl
            optim.zero_grad()
            loss.backward()
            optim.step()
            info = {"all_loss": loss.item(), "sl_loss": sl.item(), "adv_loss": adv_loss.item(), "adv_log_prob": log_prob.mean().item()}
            done += 1
            obs = nxt.detach()
            if done == 1000:
                break
    return info


def measure_rambo(ds, blocks, steps):
    rows, length, w, gamma = 256, 5, 3e-4, 0.99
    real = ReplayBuffer(len(ds["rewards"]), (OD,), np.float32, AD, np.float32, device=DEV)
    real.load_dataset(ds)
    torch.manual_seed(1)
    adam = lambda m, lr: torch.optim.Adam(m.parameters(), lr=lr)
    mk_model = lambda: EnsembleDynamicsModel(OD, AD, DYN_HID, num_ensemble=K, num_elites=E, weight_decays=DECAYS, device=DEV)
    model, tmodel = mk_model(), mk_model()
    tmodel.load_state_dict(model.state_dict())
    scaler = StandardScaler(np.zeros((1, OD + AD), np.float32), np.ones((1, OD + AD), np.float32))
    dyn = EnsembleDynamics(model, adam(model, 3e-4), scaler, termination_fn_halfcheetah)
    actor = ActorProb(MLP(OD, [256, 256]), TanhDiagGaussian(256, AD, unbounded=True, conditioned_sigma=True), DEV)
    c1, c2 = Critic(MLP(OD + AD, [256, 256]), DEV), Critic(MLP(OD + AD, [256, 256]), DEV)
    pol = RAMBOPolicy(dyn, actor, c1, c2, adam(actor, 1e-4), adam(c1, 3e-4), adam(c2, 3e-4), adam(model, 3e-4), tau=0.005, gamma=gamma,
                      alpha=0.2, adv_weight=w, adv_train_steps=steps, adv_rollout_batch_size=rows, adv_rollout_length=length, device=DEV)
    topt = adam(tmodel, 3e-4)
    mu, std = torch.zeros(OD + AD, device=DEV), torch.ones(OD + AD, device=DEV)
    last = {}

    def block(name, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "engine":
            pol._adv_train_steps = n
            last[name] = pol.update_dynamics(real)
        elif name == "device":
            pol._adv_train_steps = n
            last[name] = pol.update_dynamics_device(real)
        else:
            last[name] = torch_update_dynamics(pol, tmodel, topt, mu, std, real, n, rows, length, w, gamma)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    names = ("torch", "engine", "device")
    np.random.seed(0)
    torch.manual_seed(0)
    warm = {name: block(name, 100) for name in names}
    secs = {name: [] for name in names}
    for _ in range(blocks):
        for name in names:
            secs[name].append(block(name, steps))
    sps = {name: [steps / x for x in v] for name, v in secs.items()}
    return dict(mode="rambo_update_dynamics", steps=steps, rows=[rows, rows], rollout_length=length, adv_weight=w,
                warmup_seconds_100_steps=warm, seconds=secs, steps_per_s=sps, steps_per_s_mean={k: float(np.mean(v)) for k, v in sps.items()},
                steps_per_s_median={k: float(np.median(v)) for k, v in sps.items()},
                speedup=float(np.mean(sps["engine"]) / np.mean(sps["torch"])),
                device_over_engine_median=float(np.median(sps["device"]) / np.median(sps["engine"])),
                device_over_torch_median=float(np.median(sps["device"]) / np.median(sps["torch"])),
                device_loop_event_ms_last=float(pol.last_update_dynamics_ms),
                last_losses={k: {a: float(b) for a, b in v.items()} for k, v in last.items()})


def torch_mobile_learn(t, obs, act, nobs, rew, term, real_rows, S, coef, gamma, tau, target_entropy):
    """mobile.py:130-196 in stock torch on the GPU (auto-alpha, deterministic backup): ``t`` holds the modules and optimizers"""
    model, elites = t["model"], t["model"].elites.data
    with torch.no_grad():
        mean, logvar = model((torch.cat([obs, act], -1) - t["mu"]) / t["std"])
        mean = torch.cat([mean[..., :-1] + obs, mean[..., -1:]], -1)[elites]
        std = torch.sqrt(torch.exp(logvar))[elites]
        nxt = torch.stack([mean + torch.randn_like(std) * std for _ in range(S)], 0)[..., :-1]
        s, e, b, od = nxt.shape
        flat = nxt.reshape(-1, od)
        a_l, _ = t["actforward"](flat)
        q = torch.minimum(t["critics_old"][0](flat, a_l), t["critics_old"][1](flat, a_l)).reshape(s, e, b, 1)
        pen = q.mean(0).std(0)
        pen[:real_rows] = 0.0
        na, _ = t["actforward"](nobs)
        next_q = torch.minimum(t["critics_old"][0](nobs, na), t["critics_old"][1](nobs, na))
        target = torch.clamp((rew - coef * pen) + gamma * (1 - term) * next_q, 0, None)
    qs = torch.stack([c(obs, act) for c in t["critics"]], 0)
    critic_loss = ((qs - target) ** 2).mean()
    t["critics_optim"].zero_grad(); critic_loss.backward(); t["critics_optim"].step()
    a, logp = t["actforward"](obs)
    alpha = t["log_alpha"].detach().exp().clamp(0.0, 1.0)
    actor_loss = -torch.minimum(t["critics"][0](obs, a), t["critics"][1](obs, a)).mean() + alpha * logp.mean()
    t["actor_optim"].zero_grad(); actor_loss.backward(); t["actor_optim"].step()
    alpha_loss = -(t["log_alpha"] * (logp.detach() + target_entropy)).mean()
    t["alpha_optim"].zero_grad(); alpha_loss.backward(); t["alpha_optim"].step()
    with torch.no_grad():
        for o, n in zip(t["critics_old"].parameters(), t["critics"].parameters()):
            o.mul_(1.0 - tau).add_(n, alpha=tau)
    return {"loss/actor": actor_loss.item(), "loss/critic": critic_loss.item(), "loss/alpha": alpha_loss.item()}


def measure_mobile(ds, blocks, steps):
    from copy import deepcopy
    S, coef, gamma, tau, real_rows = 10, 1.5, 0.99, 0.005, int(B * 0.05)
    real = ReplayBuffer(len(ds["rewards"]), (OD,), np.float32, AD, np.float32, device=DEV)
    real.load_dataset(ds)
    half = len(ds["rewards"]) // 2
    fake = ReplayBuffer(half, (OD,), np.float32, AD, np.float32, device=DEV)      # model rows: any transitions do for the arithmetic
    fake.load_dataset({k: v[:half] for k, v in ds.items()})
    ring = ReplayBuffer(half, (OD,), np.float32, AD, np.float32, device=DEV)      # the same model rows as the device loop's HBM ring
    ring.reserve_device()
    ring.add_batch(ds["observations"][:half], ds["next_observations"][:half], ds["actions"][:half], ds["rewards"][:half], ds["terminals"][:half])
    torch.manual_seed(1)
    adam = lambda m, lr: torch.optim.Adam(m.parameters(), lr=lr)
    mk_model = lambda: EnsembleDynamicsModel(OD, AD, DYN_HID, num_ensemble=K, num_elites=E, weight_decays=DECAYS, device=DEV)
    model, tmodel, dmodel = mk_model(), mk_model(), mk_model()
    tmodel.load_state_dict(model.state_dict())
    dmodel.load_state_dict(model.state_dict())
    scaler = StandardScaler(np.zeros((1, OD + AD), np.float32), np.ones((1, OD + AD), np.float32))
    dyn = EnsembleDynamics(model, adam(model, 1e-3), scaler, termination_fn_halfcheetah)
    ddyn = EnsembleDynamics(dmodel, adam(dmodel, 1e-3), StandardScaler(scaler.mu, scaler.std), termination_fn_halfcheetah)
    mk_actor = lambda: ActorProb(MLP(OD, [256, 256]), TanhDiagGaussian(256, AD, unbounded=True, conditioned_sigma=True), DEV)
    mk_critics = lambda: torch.nn.ModuleList([Critic(MLP(OD + AD, [256, 256]), DEV), Critic(MLP(OD + AD, [256, 256]), DEV)])
    actor, critics = mk_actor(), mk_critics()
    tactor, tcritics = deepcopy(actor), deepcopy(critics)
    log_alpha = torch.zeros(1, requires_grad=True, device=DEV)
    pol = MOBILEPolicy(dyn, actor, critics, adam(actor, 1e-4), adam(critics, 3e-4), tau=tau, gamma=gamma,
                       alpha=(-float(AD), log_alpha, torch.optim.Adam([log_alpha], lr=1e-4)), penalty_coef=coef, num_samples=S,
                       deterministic_backup=True)
    pol.set_engine_options(seed=3)
    pol.train()
    dactor, dcritics = deepcopy(actor), deepcopy(critics)
    dla = torch.zeros(1, requires_grad=True, device=DEV)
    dpol = MOBILEDevicePolicy(ddyn, dactor, dcritics, adam(dactor, 1e-4), adam(dcritics, 3e-4), tau=tau, gamma=gamma,
                              alpha=(-float(AD), dla, torch.optim.Adam([dla], lr=1e-4)), penalty_coef=coef, num_samples=S,
                              deterministic_backup=True)
    dpol.set_engine_options(seed=3)
    dpol.train()
    event_ms = []
    tla = torch.zeros(1, requires_grad=True, device=DEV)

    def actforward(o):
        dist = tactor(o)
        sq, raw = dist.rsample()
        return sq, dist.log_prob(sq, raw)
    t = dict(model=tmodel, mu=torch.zeros(OD + AD, device=DEV), std=torch.ones(OD + AD, device=DEV), actforward=actforward, critics=tcritics,
             critics_old=deepcopy(tcritics), critics_optim=adam(tcritics, 3e-4), actor_optim=adam(tactor, 1e-4), log_alpha=tla,
             alpha_optim=torch.optim.Adam([tla], lr=1e-4))
    last = {}

    def block(name, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "device":
            last[name] = dpol.learn_n(n, real, ring, B, 0.05)
            event_ms.append(float(dpol.last_learn_n_ms))
        for _ in range(n if name != "device" else 0):
            rb, fb = real.sample(real_rows), fake.sample(B - real_rows)
            if name == "engine":
                last[name] = pol.learn({"real": rb, "fake": fb})
            else:
                mix = {k: torch.cat([rb[k], fb[k]], 0) for k in rb}
                last[name] = torch_mobile_learn(t, mix["observations"], mix["actions"], mix["next_observations"], mix["rewards"],
                                                mix["terminals"], real_rows, S, coef, gamma, tau, -float(AD))
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    names = ("torch", "engine", "device")
    np.random.seed(0)
    torch.manual_seed(0)
    warm = {name: block(name, 100) for name in names}
    del event_ms[:]
    secs = {name: [] for name in names}
    for _ in range(blocks):
        for name in names:
            secs[name].append(block(name, steps))
    sps = {name: [steps / x for x in v] for name, v in secs.items()}
    # HIP-event split of the engine's step (profiling serialises nothing here: the launches of a step are one stream already)
    pol.engine.profile_enable(True)
    n_prof = min(steps, 200)
    block("engine", n_prof)
    table = pol.engine.profile_table()
    pol.engine.profile_enable(False)
    pen_ms = sum(r["total_ms"] for r in table if "lcb" in r["name"]) / n_prof
    rest_ms = sum(r["total_ms"] for r in table if "lcb" not in r["name"]) / n_prof
    return dict(mode="mobile_learn", steps=steps, batch=B, real_rows=real_rows, num_samples=S, elites=E, penalty_rows=S * E * B,
                warmup_seconds_100_steps=warm, seconds=secs, steps_per_s=sps, steps_per_s_mean={k: float(np.mean(v)) for k, v in sps.items()},
                steps_per_s_median={k: float(np.median(v)) for k, v in sps.items()},
                speedup=float(np.mean(sps["engine"]) / np.mean(sps["torch"])),
                device_over_engine_median=float(np.median(sps["device"]) / np.median(sps["engine"])),
                device_over_torch_median=float(np.median(sps["device"]) / np.median(sps["torch"])),
                device_loop_event_ms=event_ms, device_loop_wall_ms=[1e3 * x for x in secs["device"]],
                device_loop_event_over_wall_median=float(np.median(event_ms) / (1e3 * np.median(secs["device"]))),
                engine_kernel_ms_per_step=dict(penalty_pass=pen_ms, rest=rest_ms),
                penalty_launches={r["name"]: r["total_ms"] / n_prof for r in table if "lcb" in r["name"]},
                last_losses={k: {a: float(b) for a, b in v.items()} for k, v in last.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--block-steps", type=int, default=BLOCK)
    ap.add_argument("--algos", default="mopo,combo")
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=0, help="R > 1: per-run model rings at R runs against R sequential single-run fused trainings")
    ap.add_argument("--profile-block", action="store_true", help="a warm-up and one fused MOPO block only (for a kernel trace)")
    ap.add_argument("--rambo", action="store_true", help="RAMBO's update_dynamics (engine, host loop) against its stock-torch restatement and the device loop")
    ap.add_argument("--rambo-steps", type=int, default=1000)
    ap.add_argument("--mobile", action="store_true", help="MOBILEPolicy.learn (engine, host loop) against its stock-torch restatement and MOBILEDevicePolicy.learn_n (the device loop)")
    ap.add_argument("--mobile-steps", type=int, default=500)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_throughput: no HIP device visible (the loops under test run on the GPU)")
    if a.mobile:
        res = {"shape": dict(obs=OD, act=AD, dynamics_hidden=DYN_HID, members=K, elites=E, policy_hidden=[256, 256]),
               "device": torch.cuda.get_device_name(0), "results": [measure_mobile(dataset(200_000), a.blocks, a.mobile_steps)]}
        s = json.dumps(res, indent=1)
        print(s)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(s + "\n")
        return
    if a.rambo:
        res = {"shape": dict(obs=OD, act=AD, dynamics_hidden=DYN_HID, members=K, elites=E, policy_hidden=[256, 256]),
               "device": torch.cuda.get_device_name(0), "results": [measure_rambo(dataset(200_000), a.blocks, a.rambo_steps)]}
        s = json.dumps(res, indent=1)
        print(s)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(s + "\n")
        return
    ds = dataset(DATA_ROWS)
    if a.profile_block:
        print(json.dumps(measure("mopo", ds, 1, a.block_steps, profile_only=True)))
        return
    res = {"shape": dict(obs=OD, act=AD, dynamics_hidden=DYN_HID, members=K, batch=B, rollout=ROLLOUT, model_rows=MODEL_ROWS, data_rows=DATA_ROWS),
           "device": torch.cuda.get_device_name(0), "results": [measure_runs(x, ds, a.blocks, a.block_steps, a.runs) if a.runs > 1 else measure(x, ds, a.blocks, a.block_steps)
                       for x in a.algos.split(",")]}
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()

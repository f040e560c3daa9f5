#!/usr/bin/env python3
"""Dynamics-ensemble throughput at the MOPO halfcheetah shape (17 / 6, [200] x 4, 7 members, batch 256): learn() minibatch steps/s of
the HIP engine (orl_dyn_learn_epoch) at n_runs 1 and 8, rollout rows/s of step() at 50 000 rows, and the same two measured on a stock
torch implementation written here (bmm EnsembleLinear forward, autograd, torch.optim.Adam, loss.item() per minibatch as the
reference's learn() does).  Prints one JSON object; --out writes it too."""
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
from offlinerlkit.modules import EnsembleDynamicsModel  # noqa: E402

OD, AD, HID, K, E, B = 17, 6, [200, 200, 200, 200], 7, 5, 256
DECAYS = [2.5e-5, 5e-5, 7.5e-5, 7.5e-5, 1e-4]


def engine_learn(n_runs, train_size, epochs):
    cfg = _engine.default_dyn_config(n_runs=n_runs)
    eng = _engine.Dynamics(cfg)
    torch.manual_seed(0)
    m = EnsembleDynamicsModel(OD, AD, HID, K, E, weight_decays=DECAYS)
    p = {k: v.detach().numpy() for k, v in m.state_dict().items() if k != "elites"}
    for r in range(n_runs):
        eng.set_params(r, p)
    rng = np.random.default_rng(0)
    n = train_size + 1000
    eng.load_data(rng.normal(size=(n, OD + AD)).astype(np.float32), rng.normal(size=(n, OD + 1)).astype(np.float32))
    for r in range(n_runs):
        eng.set_scaler(r, np.zeros(OD + AD, np.float32), np.ones(OD + AD, np.float32))
    idx = rng.integers(0, train_size, size=(n_runs, K, train_size))
    eng.learn_epoch(idx)                                    # warm-up (kernel loads, first-touch)
    t0 = time.perf_counter()
    for _ in range(epochs):
        loss = eng.learn_epoch(idx)
    dt = time.perf_counter() - t0
    nb = (train_size + B - 1) // B
    assert np.all(np.isfinite(loss)), loss
    eng.close()
    return dict(n_runs=n_runs, minibatches=nb * epochs, seconds=dt, minibatch_steps_per_s=nb * epochs / dt,
                run_minibatch_steps_per_s=n_runs * nb * epochs / dt)


def engine_step(rows, reps):
    eng = _engine.Dynamics(_engine.default_dyn_config())
    torch.manual_seed(0)
    m = EnsembleDynamicsModel(OD, AD, HID, K, E, weight_decays=DECAYS)
    eng.set_params(0, {k: v.detach().numpy() for k, v in m.state_dict().items() if k != "elites"})
    eng.set_scaler(0, np.zeros(OD + AD, np.float32), np.ones(OD + AD, np.float32))
    rng = np.random.default_rng(1)
    obs = rng.normal(size=(1, rows, OD)).astype(np.float32)
    act = rng.uniform(-1, 1, size=(1, rows, AD)).astype(np.float32)
    eng.step(obs, act, mode="aleatoric", coef=2.5)
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.step(obs, act, mode="aleatoric", coef=2.5)
    dt = time.perf_counter() - t0
    eng.close()
    return dict(rows=rows, seconds=dt / reps, rows_per_s=rows * reps / dt)


def torch_learn(batches):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = EnsembleDynamicsModel(OD, AD, HID, K, E, weight_decays=DECAYS, device="cuda")
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    x = torch.randn(K, batches * B, OD + AD, device=dev)
    t = torch.randn(K, batches * B, OD + 1, device=dev)

    def one(b):
        mean, logvar = m(x[:, b * B:(b + 1) * B])
        inv_var = torch.exp(-logvar)
        loss = (torch.pow(mean - t[:, b * B:(b + 1) * B], 2) * inv_var).mean(dim=(1, 2)).sum() + logvar.mean(dim=(1, 2)).sum()
        loss = loss + m.get_decay_loss() + 0.01 * m.max_logvar.sum() - 0.01 * m.min_logvar.sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.item()
    for b in range(10):
        one(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(batches):
        one(b)
    dt = time.perf_counter() - t0
    return dict(minibatches=batches, seconds=dt, minibatch_steps_per_s=batches / dt)


@torch.no_grad()
def torch_step(rows, reps):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = EnsembleDynamicsModel(OD, AD, HID, K, E, weight_decays=DECAYS, device="cuda")
    obs = torch.randn(rows, OD, device=dev)
    act = torch.rand(rows, AD, device=dev) * 2 - 1

    def one():
        mean, logvar = m(torch.cat([obs, act], -1))
        mean[..., :-1] += obs
        std = torch.sqrt(torch.exp(logvar))
        samples = mean + torch.randn_like(mean) * std
        idx = m.elites[torch.randint(0, E, (rows,), device=dev)]
        s = samples[idx, torch.arange(rows, device=dev)]
        pen = torch.amax(torch.linalg.norm(std, dim=2), dim=0)
        r = s[:, -1] - 2.5 * pen
        return s[:, :-1].cpu(), r.cpu()
    one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        one()
    dt = time.perf_counter() - t0
    return dict(rows=rows, seconds=dt / reps, rows_per_s=rows * reps / dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-size", type=int, default=256 * 400)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-epoch", action="store_true", help="one n_runs = 1 epoch of 50 minibatches only (for a kernel trace)")
    a = ap.parse_args()
    if a.profile_epoch:
        print(json.dumps(engine_learn(1, 256 * 50, 1)))
        return
    res = {"shape": dict(obs=OD, act=AD, hidden=HID, members=K, batch=B), "device": torch.cuda.get_device_name(0),
           "engine_learn": [engine_learn(1, a.train_size, a.epochs), engine_learn(8, a.train_size, a.epochs)],
           "torch_learn": torch_learn(400),
           "engine_step": engine_step(50000, 20), "torch_step": torch_step(50000, 20)}
    res["speedup_learn_R1"] = res["engine_learn"][0]["minibatch_steps_per_s"] / res["torch_learn"]["minibatch_steps_per_s"]
    res["speedup_step"] = res["engine_step"]["rows_per_s"] / res["torch_step"]["rows_per_s"]
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()

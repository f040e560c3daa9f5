#!/usr/bin/env python3
"""RCSL epoch throughput at run_rcsl.py's shape on hopper (obs 11, act 3, MLP [200] x 4 on [obs | rtg], batch 256, lr 1e-3): one
``RcslPolicy.learn_epoch`` (orl_learn_epoch: ordered gather, forward, masked MSE, backward, Adam per step, one host sync per epoch) at 1
and at 8 runs per engine, against a stock-torch restatement of the same epoch on the same GPU (torch.randperm order, index_select from
device-resident arrays, nn.Linear / ReLU forward, autograd, torch.optim.Adam, one ``.item()`` per batch like the reference's ``learn``;
R runs = R such models trained one after the other).  One invocation, alternating: a warm-up epoch of each, then ``--blocks`` timed
epochs of each, timed with a host clock around work that ends in a device synchronise.  A synthetic dataset of ``--rows`` rows (default
100 000 = 391 steps, the last batch partial).  The figure is run-steps per second.  Prints one JSON object; --out writes it too.  Needs a GPU.
``--gauss``: the same measurement of ``RcslGaussianPolicy`` at run_rcsl_gauss.py's shape (MLP [1024] x 4 down to an act_dim-wide latent, the
DiagGaussian head with a clamped state-conditioned sigma, Gaussian NLL; k_rcslg_head in place of the MSE launch)."""
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
from offlinerlkit.policy import RcslGaussianPolicy, RcslPolicy  # noqa: E402
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


def measure(ds, rows, runs, blocks, gauss=False):
    torch.manual_seed(1)
    mod = make_module(gauss)
    pol = (RcslGaussianPolicy if gauss else RcslPolicy)(None, None, mod, torch.optim.Adam(mod.parameters(), lr=LR), DEV)
    pol.set_engine_options(n_runs=runs, seed=3)
    buf = _engine.DeviceBuffer(OD, AD, 0)
    buf.load(ds["observations"], ds["actions"], ds["observations"], ds["rtgs"].reshape(rows), np.zeros(rows, np.float32))
    models = []
    for _ in range(runs):
        net = make_module(True) if gauss else MLP(input_dim=OD + 1, hidden_dims=HID, output_dim=AD).to(DEV)
        models.append((net, torch.optim.Adam(net.parameters(), lr=LR)))
    data = {k: torch.as_tensor(v, device=DEV) for k, v in ds.items()}
    engine_epoch(pol, buf, rows, runs); torch_epoch(models, data, rows)          # warm-up: graph capture / allocator
    eng, ref = [], []
    for _ in range(blocks):
        eng.append(engine_epoch(pol, buf, rows, runs))
        ref.append(torch_epoch(models, data, rows))
    return dict(runs=runs, engine_run_steps_per_s=eng, torch_run_steps_per_s=ref, engine_median=float(np.median(eng)),
                torch_median=float(np.median(ref)), speedup=float(np.median(eng) / np.median(ref)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--runs", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--gauss", action="store_true", help="RcslGaussianPolicy at run_rcsl_gauss.py's shape ([1024] x 4)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ds = dataset(a.rows)
    res = dict(policy="RcslGaussianPolicy" if a.gauss else "RcslPolicy", precision=int(os.environ.get("ORL_PRECISION", "0")),
               shape=dict(obs_dim=OD, act_dim=AD, hidden=HID_GAUSS if a.gauss else HID, batch=B, rows=a.rows, steps_per_epoch=-(-a.rows // B)),
               device=torch.cuda.get_device_name(0), results=[measure(ds, a.rows, r, a.blocks, a.gauss) for r in a.runs])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

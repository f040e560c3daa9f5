#!/usr/bin/env python3
"""Dynamics-ensemble throughput at the MOPO halfcheetah shape (17 / 6, [200] x 4, 7 members, batch 256): learn() minibatch steps/s of
the HIP engine (orl_dyn_learn_epoch) at n_runs 1 and 8, rollout rows/s of step() at 50 000 rows, and the same two measured on a stock
torch implementation written here (bmm EnsembleLinear forward, autograd, torch.optim.Adam, loss.item() per minibatch as the
reference's learn() does).  Prints one JSON object; --out writes it too.
--split: step() on device tensors at precision 0 (fp32 GEMM per layer) against precision 1 (the fused split-fp16 forward) instead.
--head: step() on device tensors with step_head 0 (k_dyn_head) against 1 (k_dyn_head_tile) at precision 0 and 1 instead."""
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


def fused_tile(rows):
    """rows per workgroup of k_dyn_fused_fwd at this shape (dyf_pick_tile: widest Kp 224, 4 fragments per wave): the largest of 64 / 32
    whose two LDS planes fit 64 KB and that still gives 256 workgroups, else 16"""
    for rt in (64, 32):
        if 4 * rt * (224 + 8) <= 65536 and -(-rows // rt) * K >= 256:
            return rt
    return 16


def ab_step(variants, rows_list, windows=5, window_s=0.4, only=None):
    """step() on device tensors by two objects of this build (variants: two dicts of config overrides), timed in alternating windows;
    every call ends in the engine's own synchronise.  Returns [(rows, reps per window [2], window means in s [2][windows])].
    only = (variant index, rows): that one engine in a plain loop, for a kernel trace."""
    torch.manual_seed(0)
    m = EnsembleDynamicsModel(OD, AD, HID, K, E, weight_decays=DECAYS)
    p = {k: v.detach().numpy() for k, v in m.state_dict().items() if k != "elites"}
    engs = {}
    for v in ((0, 1) if only is None else (only[0],)):
        engs[v] = eng = _engine.Dynamics(_engine.default_dyn_config(**variants[v]))
        eng.set_params(0, p)
        eng.set_scaler(0, np.zeros(OD + AD, np.float32), np.ones(OD + AD, np.float32))
    dev = torch.device("cuda", 0)
    out = []
    for rows in rows_list if only is None else (only[1],):
        g = torch.Generator(device=dev).manual_seed(rows)
        obs = torch.randn(1, rows, OD, device=dev, generator=g)
        act = torch.rand(1, rows, AD, device=dev, generator=g) * 2 - 1

        def window(eng, reps):
            t0 = time.perf_counter()
            for _ in range(reps):
                eng.step_device(obs, act, "aleatoric", 2.5)
            return (time.perf_counter() - t0) / reps
        for eng in engs.values():
            window(eng, 5)                                  # warm-up: code objects, workspaces grown to this row count
        if only is not None:
            window(engs[only[0]], 200)
            continue
        reps = {v: max(10, int(window_s / window(eng, 10))) for v, eng in engs.items()}
        t = {0: [], 1: []}
        for _ in range(windows):
            for v, eng in engs.items():
                t[v].append(window(eng, reps[v]))
        out.append((rows, reps, t))
    for eng in engs.values():
        eng.close()
    return out


def split_step(rows_list, windows=5, window_s=0.4, only=None):
    """precision 0 against 1 (ab_step).  Medians of `windows` windows per precision and row count."""
    out = []
    for rows, reps, t in ab_step((dict(precision=0), dict(precision=1)), rows_list, windows, window_s, only):
        med = {prec: float(np.median(v)) for prec, v in t.items()}
        out.append(dict(rows=rows, fused_rows_per_workgroup=fused_tile(rows), reps_per_window=reps, windows=windows,
                        p0_ms=med[0] * 1e3, p1_ms=med[1] * 1e3, p0_ms_windows=[x * 1e3 for x in t[0]], p1_ms_windows=[x * 1e3 for x in t[1]],
                        p0_rows_per_s=rows / med[0], p1_rows_per_s=rows / med[1], p1_over_p0_speed=med[0] / med[1]))
    return out


def head_step(precision, rows_list, windows=5, window_s=0.4, only=None):
    """step_head 0 (k_dyn_head) against 1 (k_dyn_head_tile) at one precision (ab_step): medians and ranges of `windows` windows"""
    out = []
    for rows, reps, t in ab_step((dict(precision=precision, step_head=0), dict(precision=precision, step_head=1)), rows_list, windows,
                                 window_s, only):
        med = {h: float(np.median(v)) for h, v in t.items()}
        out.append(dict(precision=precision, rows=rows, reps_per_window=reps, windows=windows, head0_ms=med[0] * 1e3, head1_ms=med[1] * 1e3,
                        head0_ms_windows=[x * 1e3 for x in t[0]], head1_ms_windows=[x * 1e3 for x in t[1]],
                        head1_over_head0_speed=med[0] / med[1]))
    return out


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
    ap.add_argument("--split", action="store_true", help="step() on device tensors at precision 0 against precision 1 (256, 12 800 and "
                    "50 000 rows); --out defaults to profiles/dyn_step_split_throughput.json")
    ap.add_argument("--split-trace", type=int, nargs=2, metavar=("PRECISION", "ROWS"), default=None,
                    help="with --split: 200 steps of one precision at one row count only (for a kernel trace: the pack launch's share)")
    ap.add_argument("--head", action="store_true", help="step() on device tensors with step_head 0 against 1 at precision 0 and 1 (256, "
                    "12 800 and 50 000 rows); --out defaults to profiles/dyn_step_head_throughput.json")
    ap.add_argument("--head-trace", type=int, nargs=3, metavar=("PRECISION", "STEP_HEAD", "ROWS"), default=None,
                    help="with --head: 200 steps of one setting at one row count only (for a kernel trace)")
    a = ap.parse_args()
    if a.head:
        if a.head_trace:
            head_step(a.head_trace[0], (), only=tuple(a.head_trace[1:]))
            return
        res = {"shape": dict(obs=OD, act=AD, hidden=HID, members=K), "device": torch.cuda.get_device_name(0),
               "what": "orl_dyn_step on device tensors, ms per call incl. its synchronise: medians of alternating windows, step_head 0 / 1",
               "step": head_step(0, (256, 12800, 50000)) + head_step(1, (256, 12800, 50000))}
        s = json.dumps(res, indent=1)
        print(s)
        out = a.out or os.path.join(ROOT, "profiles", "dyn_step_head_throughput.json")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(s + "\n")
        return
    if a.profile_epoch:
        print(json.dumps(engine_learn(1, 256 * 50, 1)))
        return
    if a.split:
        if a.split_trace:
            split_step((), only=tuple(a.split_trace))
            return
        res = {"shape": dict(obs=OD, act=AD, hidden=HID, members=K), "device": torch.cuda.get_device_name(0),
               "what": "orl_dyn_step on device tensors, ms per call incl. its synchronise: medians of alternating windows",
               "step": split_step((256, 12800, 50000))}
        s = json.dumps(res, indent=1)
        print(s)
        out = a.out or os.path.join(ROOT, "profiles", "dyn_step_split_throughput.json")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(s + "\n")
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

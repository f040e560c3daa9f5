#!/usr/bin/env python3
"""RNNDynamics throughput at the constructor-default shape on hopper (in 14, out 12, [200] x 4, 3 GRU layers, batch 256, T 20): one
``learn`` step and one ``step()`` on 256 windows on the HIP engine, and the same two on the project's own torch ``RNNModel`` with
autograd and ``torch.optim.Adam`` on the same GPU in the same call (``loss.item()`` per step, as the reference's ``learn`` does).

Method: every shape is warmed up first; a timed window is a host clock around work that ends in a device synchronise; engine and torch
windows alternate over ``--rounds`` rounds and the medians are reported with the spread.  The forward / scan / backward split of the
engine's step comes from device events (``orl_rnn_profile``), in windows of their own.  Prints one JSON object; --out writes it too.

``--runs R [R ...]`` measures the multi-run objects instead: one ``step_runs`` of an R-run engine against R one-run engines stepped one
after the other (same GPU, same call, same alternating windows and medians), with the device events of the R-run step and of a
one-run step beside them (``profiles/rnn_throughput_runs.json`` holds R = 1, 2, 4, 8, 16).

``--rollout`` measures ONE model step of a rollout of 256 trajectories four ways (same GPU, same call, same alternating windows and
medians): (a) ``step_device`` on the carried state, (b) the engine's ``forward`` on device tensors at T = 1 (what there was for that
step before the carried state: no history, so not the same model output), (c) ``step`` on 20-step windows, (d) the torch ``RNNModel``
in eval mode with ``h_state`` carried; and one ``rollout_device`` of 256 trajectories x 200 steps with an untrained
``AutoregressivePolicy`` (``profiles/rnn_rollout_throughput.json``)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "offlinerl-kit_amd"))
from offlinerlkit import _engine  # noqa: E402
from offlinerlkit.dynamics import RNNDynamics  # noqa: E402
from offlinerlkit.nets import RNNModel  # noqa: E402
from offlinerlkit.utils.scaler import StandardScaler  # noqa: E402

IN, OUT, HID, L, P_DROP, B, T = 14, 12, [200, 200, 200, 200], 3, 0.1, 256, 20
OBS = OUT - 1


def data(n, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, T, IN)).astype(np.float32), rng.normal(size=(n, T, OUT)).astype(np.float32),
            (rng.uniform(size=(n, T)) < 0.9).astype(np.float32))


def window(fn, sync):
    sync()
    t0 = time.perf_counter()
    n = fn()
    sync()
    return (time.perf_counter() - t0) / n


def summary(xs):
    return dict(median_ms=1e3 * statistics.median(xs), min_ms=1e3 * min(xs), max_ms=1e3 * max(xs), windows=len(xs))


def emit(res, out):
    s = json.dumps(res, indent=1)
    print(s)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(s + "\n")


def main_runs(a):
    """--runs: one ``step_runs`` of an R-run object against R one-run objects stepped one after the other, for every R given; same
    data set, run r on rows of its own, same method as the rest of the tool (alternating windows, medians)"""
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)                                   # noqa: E731
    x, tg, mk = data(4 * B)
    res = {"shape": dict(input_dim=IN, output_dim=OUT, hidden=HID, rnn_num_layers=L, dropout=P_DROP, batch=B, T=T),
           "device": torch.cuda.get_device_name(0), "steps_per_window": a.batches, "runs": {}}
    for R in a.runs:
        many = _engine.RnnDynamicsEngine(_engine.default_rnn_config(n_runs=R))
        ones = [_engine.RnnDynamicsEngine(_engine.default_rnn_config(seed=r)) for r in range(R)]
        for r in range(R):
            torch.manual_seed(r)
            init = {k: v.numpy() for k, v in RNNModel(IN, OUT, HID, L, P_DROP).state_dict().items()}
            many.set_params(init, run=r)
            ones[r].set_params(init)
        for e in [many] + ones:
            e.load_data(x, tg, mk)
        idx = np.stack([np.random.default_rng(100 + r).permutation(4 * B)[:B] for r in range(R)]).astype(np.int64)

        def many_steps():
            for _ in range(a.batches):
                losses = many.step_runs(idx)
            assert np.isfinite(losses).all()
            return a.batches

        def one_steps():
            for _ in range(a.batches):
                losses = [ones[r].step(idx[r]) for r in range(R)]
            assert np.isfinite(losses).all()
            return a.batches

        fns = {"step_runs": many_steps, "one_run_steps": one_steps}
        for fn in fns.values():
            fn()
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append(window(fn, sync))
        row = {k: summary(v) for k, v in times.items()}
        row["ratio_one_run_steps_over_step_runs"] = row["one_run_steps"]["median_ms"] / row["step_runs"]["median_ms"]
        for name, e in (("step_runs_split_ms", many), ("one_run_step_split_ms", ones[0])):      # device events, in windows of their own
            e.profile(True)
            splits = []
            for _ in range(a.rounds):
                e.step_runs(idx) if e is many else e.step(idx[0])
                splits.append(e.profile_read())
            e.profile(False)
            row[name] = {k: statistics.median(s[k] for s in splits) for k in splits[0]}
        res["runs"][str(R)] = row
        for e in [many] + ones:
            e.close()
    emit(res, a.out)


def main_rollout(a):
    """--rollout: one model step of 256 trajectories through the carried state against the other ways to make it, and a whole
    ``rollout_device``"""
    from offlinerlkit.modules import RcslModule
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import AutoregressivePolicy, RcslPolicy
    from offlinerlkit.utils.termination_fns import termination_fn_default
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)                                   # noqa: E731
    act_dim, horizon = IN - OBS, 200
    torch.manual_seed(0)
    model = RNNModel(IN, OUT, HID, L, P_DROP)
    with torch.no_grad():                                                        # small steps: 200 of them stay finite
        model.output_layer.weight.mul_(0.01)
        model.output_layer.bias.zero_()
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    dyn = RNNDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), StandardScaler(np.zeros((1, IN), np.float32), np.ones((1, IN), np.float32)),
                      termination_fn_default)
    x, _, _ = data(B)
    obss, acts = x[:, :, :OBS].copy(), x[:, :, OBS:].copy()
    obs_d, act_d, x1_d = (torch.as_tensor(v, device=dev).contiguous() for v in (obss[:, -1], acts[:, -1], x[:, -1:]))
    dyn.step(obss, acts)                                                         # binds the engine for 20-step windows
    dyn.reset_state(B)
    tm = RNNModel(IN, OUT, HID, L, P_DROP, device="cuda")
    tm.load_state_dict(init)
    tm.eval()

    def step_device():
        for _ in range(a.batches):
            dyn.step_device(obs_d, act_d)
        return a.batches

    def forward_t1():
        for _ in range(a.batches):
            dyn._eng.forward(x1_d)
        return a.batches

    def step_windows():
        for _ in range(a.batches):
            dyn.step(obss, acts)
        return a.batches

    @torch.no_grad()
    def torch_carried():
        h = None
        for _ in range(a.batches):
            pred, h = tm(x1_d, h)
            pred[:, -1, :-1] + obs_d
        return a.batches

    runs = {"a_step_device": step_device, "b_engine_forward_T1_device": forward_t1, "c_step_20_step_windows": step_windows,
            "d_torch_eval_h_state_carried": torch_carried}
    for fn in runs.values():
        fn()
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            times[k].append(window(fn, sync))
    res = {"shape": dict(input_dim=IN, output_dim=OUT, hidden=HID, rnn_num_layers=L, rows=B, window_T=T),
           "device": torch.cuda.get_device_name(0), "steps_per_window": a.batches, "model_step": {k: summary(v) for k, v in times.items()}}
    ms = res["model_step"]
    res["ratio_b_over_a"] = ms["b_engine_forward_T1_device"]["median_ms"] / ms["a_step_device"]["median_ms"]
    res["ratio_c_over_a"] = ms["c_step_20_step_windows"]["median_ms"] / ms["a_step_device"]["median_ms"]
    res["ratio_d_over_a"] = ms["d_torch_eval_h_state_carried"]["median_ms"] / ms["a_step_device"]["median_ms"]
    # one whole rollout: 256 trajectories x 200 steps, nothing terminates
    mod = RcslModule(MLP(input_dim=OBS + 1, hidden_dims=[32, 32], output_dim=act_dim), "cuda:0")
    pol = RcslPolicy(dyn, AutoregressivePolicy(OBS, act_dim, [200, 200], 1e-3, "cuda:0"), mod, torch.optim.Adam(mod.parameters(), lr=1e-3), "cuda:0")
    store = _engine.TrajStore(OBS, act_dim, B, B * horizon)
    init_obs = obss[:, 0].copy()

    def rollout():
        _, info = pol.rollout_device(init_obs, horizon, store=store)
        assert info["num_transitions"] == B * horizon and np.isfinite(info["reward_mean"])
        return 1

    rollout()
    roll = [window(rollout, sync) for _ in range(a.rounds)]
    res["rollout_device_256x200"] = summary(roll)
    res["rollout_device_256x200"]["ms_per_model_step"] = res["rollout_device_256x200"]["median_ms"] / horizon
    emit(res, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20, help="optimizer steps per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, nargs="+", default=None, metavar="R",
                    help="instead: one step_runs of an R-run object against R one-run objects stepped in turn, for every R given")
    ap.add_argument("--rollout", action="store_true",
                    help="instead: one model step through the carried state (step_device) against forward at T = 1, step() on 20-step "
                         "windows and the torch model with h_state carried, and one rollout_device of 256 x 200")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnn_throughput.py measures on the GPU: no HIP device visible")
    if a.runs:
        return main_runs(a)
    if a.rollout:
        return main_rollout(a)
    dev = torch.device("cuda", 0)
    x, tg, mk = data(a.batches * B)
    sync = lambda: torch.cuda.synchronize(dev)                                   # noqa: E731

    # the engine: an epoch of `batches` steps in one call (one host synchronisation), and learn() / step() through the class
    torch.manual_seed(0)
    model = RNNModel(IN, OUT, HID, L, P_DROP)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    eng = _engine.RnnDynamicsEngine(_engine.default_rnn_config())
    eng.set_params({k: v.numpy() for k, v in init.items()})
    eng.load_data(x, tg, mk)
    order = np.arange(a.batches * B, dtype=np.int64)
    dyn = RNNDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), StandardScaler(np.zeros((1, IN), np.float32), np.ones((1, IN), np.float32)),
                      lambda o, ac, n: np.zeros((len(o), 1), bool))
    obss, acts = x[:B, :, :OBS].copy(), x[:B, :, OBS:].copy()

    # the torch baseline
    tm = RNNModel(IN, OUT, HID, L, P_DROP, device="cuda")
    tm.load_state_dict(init)
    opt = torch.optim.Adam(tm.parameters(), lr=1e-3)
    xd, td, md = (torch.as_tensor(v, device=dev) for v in (x, tg, mk))

    def torch_learn():
        tm.train()
        for b in range(a.batches):
            s = slice(b * B, (b + 1) * B)
            pred, _ = tm(xd[s])
            loss = (((pred - td[s]) ** 2).mean(-1) * md[s]).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            loss.item()
        return a.batches

    @torch.no_grad()
    def torch_step():
        tm.eval()
        for _ in range(a.batches):
            pred, _ = tm(xd[:B])
            last = pred[:, -1].cpu().numpy()
            last[:, :-1] + obss[:, -1]
        return a.batches

    def engine_epoch():
        losses = eng.learn_epoch(order)
        assert np.isfinite(losses).all()
        return a.batches

    def class_learn():
        for b in range(a.batches):
            s = slice(b * B, (b + 1) * B)
            dyn.learn((x[s], tg[s], mk[s]))
        return a.batches

    def class_step():
        for _ in range(a.batches):
            dyn.step(obss, acts)
        return a.batches

    runs = {"engine_learn_epoch_step": engine_epoch, "class_learn_call": class_learn, "torch_learn_step": torch_learn,
            "class_step_256_windows": class_step, "torch_step_256_windows": torch_step}
    for fn in runs.values():                                                     # warm-up: code objects, first touch, library choices
        fn()
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            times[k].append(window(fn, sync))
    res = {"shape": dict(input_dim=IN, output_dim=OUT, hidden=HID, rnn_num_layers=L, dropout=P_DROP, batch=B, T=T),
           "device": torch.cuda.get_device_name(0), "steps_per_window": a.batches}
    res.update({k: summary(v) for k, v in times.items()})
    eng.profile(True)
    splits = []
    for _ in range(a.rounds):
        eng.learn_epoch(order)
        splits.append(eng.profile_read())
    eng.profile(False)
    res["engine_step_split_ms"] = {k: statistics.median(s[k] for s in splits) for k in splits[0]}
    res["learn_ratio_torch_over_engine"] = res["torch_learn_step"]["median_ms"] / res["engine_learn_epoch_step"]["median_ms"]
    res["step_ratio_torch_over_engine"] = res["torch_step_256_windows"]["median_ms"] / res["class_step_256_windows"]["median_ms"]
    eng.close()
    emit(res, a.out)


if __name__ == "__main__":
    main()

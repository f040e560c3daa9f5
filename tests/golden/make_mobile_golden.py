#!/usr/bin/env python3
"""Golden vectors for MOBILE (csrc/algo_mobile.inc, orl_dynsample_next, offlinerlkit.policy.MOBILEPolicy) from the REAL reference's
``MOBILEPolicy.learn`` / ``compute_lcb`` (policy/model_based/mobile.py:130-196) on the reference's ``EnsembleDynamics.sample_next_obss``
(dynamics/ensemble_dynamics.py:82-99) and ``EnsembleDynamicsModel``, run on the CPU.  Usage: make_mobile_golden.py <reference root>.

The reference is imported as in make_rambo_golden.py (gym, the dynamics package and the logger stubbed; policy files, modules and the MLP
from the tree as they are).  Inputs are mobile_cases.py's synthetic arrays; the draws are teacher-forced through make_golden's
NoiseFeeder (``torch.randn_like`` per sample of ``sample_next_obss``, then the three ``rsample`` draws).  The samples, the penalty and
the un-clamped target are read from the locals of the reference's own frames when they return.

Per fixture and step: the logged losses, q1 / q2 / target_q / penalty / lcb_q; at step 0 the samples (digest; full for the tiny cases);
post-step parameters (full for the tiny cases, digests for the larger ones); the state_dict key inventory.

Asserted here, so that the fixtures cannot pass vacuously: in every case the clamp at 0 is active on 10 % .. 90 % of the rows of step 0,
the penalty of every model row is above 1e-3 of the Q scale (max |lcb_q|), and the penalty of every real row is exactly 0."""
import importlib
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.dont_write_bytecode = True
import synth  # noqa: E402
import make_golden as mg  # noqa: E402
import make_rambo_golden as mr  # noqa: E402
import mobile_cases as mc  # noqa: E402

NETS = (("actor", lambda p: p.actor), ("critic1", lambda p: p.critics[0]), ("critic2", lambda p: p.critics[1]),
        ("critic1_old", lambda p: p.critics_old[0]), ("critic2_old", lambda p: p.critics_old[1]))


def import_reference(root):
    ns = mr.import_reference(root)
    ns.MOBILEPolicy = importlib.import_module("offlinerlkit.policy.model_based.mobile").MOBILEPolicy
    return ns


def build(ns, c, st, dyn_st, scaler):
    dm, sc, ed = ns.dyn
    od, ad, hid = c["obs_dim"], c["act_dim"], c["hidden"]
    model = dm.EnsembleDynamicsModel(od, ad, c["dyn_hidden"], c["K"], len(c["elite_idx"]), weight_decays=[0.0] * (len(c["dyn_hidden"]) + 1))
    with torch.no_grad():
        params = dict(model.named_parameters())
        for k, v in dyn_st.items():
            assert tuple(params[k].shape) == v.shape, (k, params[k].shape, v.shape)
            params[k].copy_(torch.from_numpy(v))
    model.set_elites(list(c["elite_idx"]))
    dyn = ed.EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), sc.StandardScaler(scaler[0], scaler[1]),
                              lambda o, a, n: np.zeros((len(o), 1), bool))
    actor = ns.ActorProb(ns.MLP(od, hid), ns.TanhDiagGaussian(hid[-1], ad, unbounded=True, conditioned_sigma=True), "cpu")
    critics = torch.nn.ModuleList([ns.Critic(ns.MLP(od + ad, hid), "cpu"), ns.Critic(ns.MLP(od + ad, hid), "cpu")])
    mg._load(actor, st["actor"]); mg._load(critics[0], st["critic1"]); mg._load(critics[1], st["critic2"])
    cfg = mc.oracle_cfg(c)
    if cfg["auto_alpha"]:
        log_alpha = torch.tensor(st["log_alpha"].copy(), requires_grad=True)
        alpha = (cfg["target_entropy"], log_alpha, torch.optim.Adam([log_alpha], lr=cfg["alpha_lr"]))
    else:
        alpha = cfg["alpha"]
    pol = ns.MOBILEPolicy(dyn, actor, critics, torch.optim.Adam(actor.parameters(), lr=cfg["actor_lr"]),
                          torch.optim.Adam(critics.parameters(), lr=cfg["critic_lr"]), tau=cfg["tau"], gamma=cfg["gamma"], alpha=alpha,
                          penalty_coef=c["penalty_coef"], num_samples=c["S"], deterministic_backup=c["det"])
    mg._load(pol.critics_old[0], st["critic1_old"]); mg._load(pol.critics_old[1], st["critic2_old"])
    return pol


def gen(ns, case):
    c, st, dyn_st, scaler, batches, noises = mc.case_inputs(case)
    pol = build(ns, c, st, dyn_st, scaler)
    pol.train()
    full = "tiny" in case
    rec1, rec2 = mg.CallRecorder(pol.critics[0]), mg.CallRecorder(pol.critics[1])
    feeder = mg.NoiseFeeder(); feeder.install()
    grabbed = {}

    def prof(frame, event, arg):
        if event != "return":
            return
        name, loc = frame.f_code.co_name, frame.f_locals
        if name == "sample_next_obss" and "next_obss" in loc:
            grabbed["samples"] = loc["next_obss"].detach().numpy().copy()
        elif name == "compute_lcb" and "penalty" in loc:
            grabbed["lcb"] = loc["penalty"].detach().numpy().copy()
            grabbed["lcb_q"] = loc["pred_next_qs"].detach().numpy().copy()
        elif name == "learn" and "target_q" in loc and "next_q" in loc:
            grabbed["penalty"] = loc["penalty"].detach().numpy().copy()
            grabbed["target_q"] = loc["target_q"].detach().numpy().copy()
            raw = (loc["rewards"] - pol._penalty_coef * loc["penalty"]) + pol._gamma * (1 - loc["terminals"]) * loc["next_q"]
            grabbed["raw_target"] = raw.detach().numpy().copy()

    out = OrderedDict(); keys = None
    out["state_keys"] = np.array(list(pol.state_dict().keys()))
    try:
        for k, (b, n) in enumerate(zip(batches, noises)):
            feeder.normal_q = [n["dyn"][s] for s in range(c["S"])] + [n["eps_lcb"], n["eps_next"], n["eps_actor"]]
            rec1.outs.clear(); rec2.outs.clear(); grabbed.clear()
            sys.setprofile(prof)
            try:
                res = pol.learn(mr_tb2(b))
            finally:
                sys.setprofile(None)
            assert not feeder.normal_q
            keys = keys or list(res.keys())
            tag = f"step{k}"
            out[f"{tag}/losses"] = np.array([res[x] for x in keys], dtype=np.float64)
            out[f"{tag}/q1"], out[f"{tag}/q2"] = rec1.outs[0], rec2.outs[0]          # critic(obss, actions): the first call of learn()
            out[f"{tag}/target_q"], out[f"{tag}/penalty"] = grabbed["target_q"], grabbed["penalty"]
            out[f"{tag}/lcb_q"] = grabbed["lcb_q"].reshape(-1, 1)
            B_real, B = c["B_real"], c["B_real"] + c["B_fake"]
            qscale = float(np.abs(grabbed["lcb_q"]).max())
            clamped = float((grabbed["raw_target"] < 0).mean())
            pen = grabbed["penalty"].reshape(-1)
            assert np.array_equal(grabbed["target_q"], np.where(grabbed["raw_target"] < 0, 0, grabbed["raw_target"]).astype(np.float32))
            assert pen.shape == (B,) and np.all(pen[:B_real] == 0), pen[:B_real]
            assert np.all(pen[B_real:] > 1e-3 * qscale), (pen[B_real:].min(), qscale)
            if k == 0:
                assert 0.10 <= clamped <= 0.90, clamped
                assert np.any(grabbed["target_q"] == 0)
                out["step0/samples/digest"] = synth.digest(grabbed["samples"])
                if full:
                    out["step0/samples/full"] = grabbed["samples"]
                out["step0/clamped_fraction"] = np.array([clamped])
            print(f"{case} step {k}: clamp active on {clamped:.3f} of the rows, penalty of the model rows in "
                  f"[{pen[B_real:].min():.4g}, {pen[B_real:].max():.4g}], Q scale {qscale:.4g}")
            if k in (0, len(batches) - 1):
                for nm, get in NETS:
                    mg._put_state(out, f"state{k}/{nm}", mg._state_of(get(pol)), full)
                if pol._is_auto_alpha:
                    out[f"state{k}/log_alpha"] = pol._log_alpha.detach().numpy().copy()
    finally:
        feeder.uninstall()
    out["loss_keys"] = np.array(keys)
    return out


def mr_tb2(b):
    return {part: {k: torch.tensor(v) for k, v in b[part].items()} for part in ("real", "fake")}


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("OFFLINERLKIT_REF", "")
    ns = import_reference(root)
    torch.set_num_threads(4)
    for case in mc.CASES:
        out = gen(ns, case)
        path = os.path.join(HERE, f"{case}.npz")
        np.savez_compressed(path, **out)
        print("wrote", case, len(out), "arrays,", os.path.getsize(path), "bytes")

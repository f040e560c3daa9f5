#!/usr/bin/env python3
"""Golden vectors for RAMBO's advantage (csrc/kernels.h k_adv_norm, orl_engine_adv_advantage) from the REAL reference's
``RAMBOPolicy.dynamics_step_and_forward`` (policy/model_based/rambo.py:164-181), run on the CPU.
Usage: make_rambo_adv_golden.py <reference root>.

The set-up is make_rambo_golden.py's TINY (obs 3, act 2, policy [16, 16], 37 rollout + 29 dataset rows) with the reference's
``termination_fn_hopper`` as the dynamics' terminal function (it reads observation columns 0 and 1, so it is well defined from
obs_dim 2).  The rollout rows are shifted to where that test discriminates -- height around its 0.7 threshold, a small angle -- and
the fed model noise is scaled down, so that the reference marks at least a quarter of the rows of every step terminal and at least a
quarter not (asserted).  Two consecutive steps (the next observations feed the next call) for ``include_ent_in_adv`` False and True.

rambo_adv_tiny.npz holds arrays only: the actor's and the critics' parameters, and per trajectory ``ent0`` / ``ent1`` and step the
rows (obs, act), the reference's next_obs and reward, and -- read from the locals of the reference's own frame when it returns -- the
terminals, next_policy_log_prob, next_q, value, value_baseline, the raw advantage (value - value_baseline, the frame's own fp32
tensors) and the normalised one, and the five logged values.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_dyn_golden as mk  # noqa: E402
import make_rambo_golden as mr  # noqa: E402

TINY = dict(mr.TINY, steps=2, noise_scale=0.12)
TERM_KIND_HOPPER = 2      # the code of orl_buffer_append_rollout / utils.termination_fns.TERM_HOPPER


def shifted_rows(c, t):
    """make_rambo_golden's rows of call ``t`` with the rollout observations moved to the hopper test's thresholds"""
    d = mr.step_inputs(c, t)
    rng = np.random.default_rng(c["seed"] * 1000 + t)
    Ba = c["Ba"]
    d["obs"][:, 0] = (0.7 + 0.25 * rng.normal(size=Ba)).astype(np.float32)
    d["obs"][:, 1] = (0.1 * rng.normal(size=Ba)).astype(np.float32)
    d["eps"] = (d["eps"] * c["noise_scale"]).astype(np.float32)
    return d


def run(ns, c, include_ent, term_fn):
    model, dyn, pol, _ = mr.build(ns, c, 1.0)
    dyn.terminal_fn = term_fn
    pol._include_ent_in_adv = bool(include_ent)
    out, queue, grabbed = {}, [], {}
    orig_normal = torch.normal

    def fed_normal(mean, std, *a, **k):
        eps = queue.pop(0)
        assert tuple(eps.shape) == tuple(mean.shape), (eps.shape, mean.shape)
        return (eps * std).add(mean)

    def prof(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "dynamics_step_and_forward":
            loc = frame.f_locals
            f = lambda x: x.detach().numpy().copy().reshape(-1)
            grabbed.update(terminals=np.asarray(loc["terminals"]).reshape(-1).copy(), logp_next=f(loc["next_policy_log_prob"]),
                           next_q=f(loc["next_q"]), value=f(loc["value"]), value_baseline=f(loc["value_baseline"]),
                           raw=f(loc["value"] - loc["value_baseline"]), advantage=f(loc["advantage"]), reward=f(loc["rewards"]))

    np.random.seed(c["seed"] + 3)
    torch.normal = fed_normal
    try:
        obs = None
        for t in range(c["steps"]):
            d = shifted_rows(c, t)
            if obs is not None:
                d["obs"] = obs
            queue.append(torch.from_numpy(d["eps"]))
            sys.setprofile(prof)
            try:
                nxt, term, info = pol.dynamics_step_and_forward(d["obs"], d["act"], *(torch.from_numpy(d[k]) for k in
                                                                                  ("sl_obs", "sl_act", "sl_next_obs", "sl_rew")))
            finally:
                sys.setprofile(None)
            frac = float(np.mean(term))
            print(f"include_ent {include_ent} step {t}: terminal fraction {frac:.3f}")
            assert 0.25 <= frac <= 0.75, frac
            assert np.array_equal(np.asarray(term).reshape(-1), grabbed["terminals"])
            tag = f"step{t}"
            out[f"{tag}/obs"], out[f"{tag}/act"], out[f"{tag}/next_obs"] = d["obs"], d["act"], nxt.astype(np.float32)
            out[f"{tag}/reward"] = grabbed["reward"]
            out[f"{tag}/terminals"] = grabbed["terminals"].astype(np.float32)
            for k in ("logp_next", "next_q", "value", "value_baseline", "raw", "advantage"):
                out[f"{tag}/{k}"] = grabbed[k]
            out[f"{tag}/losses"] = np.array([info["adv_dynamics_update/" + k] for k in mr.LOSS_KEYS], np.float64)
            obs = nxt.copy()
    finally:
        torch.normal = orig_normal
    nets = {"actor": pol.actor, "critic1": pol.critic1, "critic2": pol.critic2}
    params = {f"{n}/{k}": v.detach().numpy().copy() for n, m in nets.items() for k, v in m.state_dict().items()}
    return out, params


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("OFFLINERLKIT_REF", "")
    ns = mr.import_reference(root)
    tf = mk._load_file("offlinerlkit.utils.termination_fns", os.path.join(root, "offlinerlkit/utils/termination_fns.py"))
    torch.set_num_threads(4)
    out = {"gamma": np.float32(TINY["gamma"]), "alpha": np.float32(TINY["alpha"]), "term_kind": np.int32(TERM_KIND_HOPPER)}
    for ent in (0, 1):
        steps, params = run(ns, TINY, ent, tf.termination_fn_hopper)
        out.update({f"ent{ent}/{k}": v for k, v in steps.items()})
        if ent == 0:
            out.update(params)
        else:      # both trajectories start from the same seeds: the same nets
            assert all(np.array_equal(out[k], v) for k, v in params.items())
    path = os.path.join(HERE, "rambo_adv_tiny.npz")
    np.savez_compressed(path, **out)
    print("rambo_adv_tiny.npz", os.path.getsize(path))

#!/usr/bin/env python3
"""Golden vectors for RAMBO's adversarial model update (csrc/dynamics.hip orl_dynadv_*, offlinerlkit.policy.RAMBOPolicy) from the REAL
reference's ``RAMBOPolicy.dynamics_step_and_forward`` (policy/model_based/rambo.py:129-207) on the reference's ``EnsembleDynamics`` /
``EnsembleDynamicsModel``, run on the CPU.  Usage: make_rambo_golden.py <reference root>.

gym, the reference's dynamics package and its logger are stubbed as in make_dyn_golden.py; the policy files (base_policy, sac, mopo,
rambo), the actor / critic modules and the MLP are loaded from the reference tree as they are.  The draws are fed and recorded:
``Normal.sample`` goes through ``torch.normal(loc, scale)``, which is replaced by ``eps * scale + loc`` on a queued fp32 ``eps`` (the
operations torch.normal itself applies to its own draw); ``random_elite_idxs`` is wrapped to record its ``np.random.choice``; the rows
are drawn here.  ``log_prob``, ``advantage`` and the per-member log-probabilities are read from the locals of the reference's own
frame when it returns.

Fixtures:
  rambo_tiny.npz   obs 3, act 2, [32, 32], 3 members, elites [2, 0] (member 1 is no elite), nonzero decays, 37 rollout + 29 dataset
                   rows, adv_weight 1: three consecutive calls (the next observations feed the next call) with, per step, the inputs,
                   eps, model indices, sample, log_prob, advantage, the five logged values, full parameters, the max / min_logvar
                   gradients (all gradients at step 0) and the adversarial Adam state; trajectory ``w0`` is the same with adv_weight 0
  rambo_mopo.npz   17 / 6, [200] x 4, 7 members, 5 elites, 256 + 256 rows, the launcher's adv_weight 3e-4: one step, the logged
                   values, log_prob, advantage and parameter digests (inputs and eps are regenerated from the seed: ``step_inputs``)
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import synth  # noqa: E402
import make_dyn_golden as mk  # noqa: E402

TINY = dict(obs_dim=3, act_dim=2, hidden=[32, 32], K=3, elites=2, elite_idx=[2, 0], decays=[1e-4, 2.5e-4, 5e-4], Ba=37, Bs=29, steps=3,
            seed=41, lr=1e-3, adv_lr=1e-3, pol_hidden=[16, 16], gamma=0.99, alpha=0.2)
MOPO = dict(obs_dim=17, act_dim=6, hidden=[200, 200, 200, 200], K=7, elites=5, elite_idx=[6, 1, 3, 0, 4],
            decays=[2.5e-5, 5e-5, 7.5e-5, 7.5e-5, 1e-4], Ba=256, Bs=256, steps=1, seed=42, lr=1e-3, adv_lr=3e-4, pol_hidden=[32, 32],
            gamma=0.99, alpha=0.2, adv_weight=3e-4)
LOSS_KEYS = ("all_loss", "sl_loss", "adv_loss", "adv_advantage", "adv_log_prob")


def import_reference(root):
    """make_dyn_golden's stubs plus the policy side: a package shell for offlinerlkit.policy whose submodules come from the tree"""
    ref = mk.import_reference(root)
    gym = types.ModuleType("gym")
    gym.spaces = types.ModuleType("gym.spaces")
    gym.spaces.Space, gym.Env = type("Space", (), {}), type("Env", (), {})
    sys.modules["gym"], sys.modules["gym.spaces"] = gym, gym.spaces
    for pkg in ("policy", "modules", "nets"):
        m = sys.modules.get("offlinerlkit." + pkg) or types.ModuleType("offlinerlkit." + pkg)
        m.__path__ = [os.path.join(root, "offlinerlkit", pkg)]
        sys.modules["offlinerlkit." + pkg] = m
    sys.modules["offlinerlkit.utils"].scaler = sys.modules["offlinerlkit.utils.scaler"]
    pol = sys.modules["offlinerlkit.policy"]
    pol.BasePolicy = importlib.import_module("offlinerlkit.policy.base_policy").BasePolicy
    pol.SACPolicy = importlib.import_module("offlinerlkit.policy.model_free.sac").SACPolicy
    pol.MOPOPolicy = importlib.import_module("offlinerlkit.policy.model_based.mopo").MOPOPolicy
    ns = types.SimpleNamespace(dyn=ref)
    ns.RAMBOPolicy = importlib.import_module("offlinerlkit.policy.model_based.rambo").RAMBOPolicy
    ns.MLP = importlib.import_module("offlinerlkit.nets.mlp").MLP
    ns.ActorProb = importlib.import_module("offlinerlkit.modules.actor_module").ActorProb
    ns.Critic = importlib.import_module("offlinerlkit.modules.critic_module").Critic
    ns.TanhDiagGaussian = importlib.import_module("offlinerlkit.modules.dist_module").TanhDiagGaussian
    return ns


def scaler_fit_rows(c):
    rng = np.random.default_rng(c["seed"] + 1)
    return (rng.normal(size=(300, c["obs_dim"] + c["act_dim"])) * 1.5 + 0.25).astype(np.float32)


def step_inputs(c, t):
    """the rows and the eps of call ``t`` (the rollout observations of calls t > 0 are the previous call's next observations)"""
    rng = np.random.default_rng(c["seed"] * 100 + t)
    od, ad, Ba, Bs, K = c["obs_dim"], c["act_dim"], c["Ba"], c["Bs"], c["K"]
    d = {"obs": rng.normal(size=(Ba, od)).astype(np.float32), "act": rng.uniform(-1, 1, size=(Ba, ad)).astype(np.float32),
         "sl_obs": rng.normal(size=(Bs, od)).astype(np.float32), "sl_act": rng.uniform(-1, 1, size=(Bs, ad)).astype(np.float32)}
    d["sl_next_obs"] = (d["sl_obs"] + 0.3 * rng.normal(size=(Bs, od))).astype(np.float32)
    d["sl_rew"] = rng.normal(size=(Bs, 1)).astype(np.float32)
    d["eps"] = rng.normal(size=(K, Ba, od + 1)).astype(np.float32)
    return d


def build(ns, c, adv_weight):
    dm, sc, ed = ns.dyn
    torch.manual_seed(c["seed"])
    model = dm.EnsembleDynamicsModel(c["obs_dim"], c["act_dim"], c["hidden"], c["K"], c["elites"], weight_decays=c["decays"])
    model.set_elites(c["elite_idx"])
    dyn = ed.EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=c["lr"]), sc.StandardScaler(),
                              lambda o, a, n: np.zeros((len(o), 1), bool))
    dyn.scaler.fit(scaler_fit_rows(c))
    torch.manual_seed(c["seed"] + 7)
    od, ad, hid = c["obs_dim"], c["act_dim"], c["pol_hidden"]
    actor = ns.ActorProb(ns.MLP(od, hid), ns.TanhDiagGaussian(hid[-1], ad, unbounded=True, conditioned_sigma=True), "cpu")
    c1, c2 = ns.Critic(ns.MLP(od + ad, hid), "cpu"), ns.Critic(ns.MLP(od + ad, hid), "cpu")
    adv_optim = torch.optim.Adam(model.parameters(), lr=c["adv_lr"])
    pol = ns.RAMBOPolicy(dyn, actor, c1, c2, torch.optim.Adam(actor.parameters(), lr=1e-4), torch.optim.Adam(c1.parameters(), lr=3e-4),
                         torch.optim.Adam(c2.parameters(), lr=3e-4), adv_optim, gamma=c["gamma"], alpha=c["alpha"], adv_weight=adv_weight,
                         adv_rollout_batch_size=c["Ba"], device="cpu")
    return model, dyn, pol, adv_optim


def run_steps(ns, c, adv_weight, full):
    """-> ({key: array}, [per-step dict of every parameter's gradient], smallest over rows of the largest elite lp_k)"""
    model, dyn, pol, adv_optim = build(ns, c, adv_weight)
    out = {}
    mk.put_state(out, "init", mk.state(model), full)
    out["scaler_mu"], out["scaler_std"] = dyn.scaler.mu, dyn.scaler.std
    queue, picked, grabbed = [], [], {}
    orig_normal, orig_idxs = torch.normal, model.random_elite_idxs

    def fed_normal(mean, std, *a, **k):
        eps = queue.pop(0)
        assert tuple(eps.shape) == tuple(mean.shape), (eps.shape, mean.shape)
        return (eps * std).add(mean)

    def rec_idxs(n):
        idx = orig_idxs(n)
        picked.append(np.asarray(idx).copy())
        return idx

    def prof(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "dynamics_step_and_forward":
            loc = frame.f_locals
            lp = loc["dist"].log_prob(loc["sample"]).sum(-1)[model.elites.data]
            grabbed.update(log_prob=loc["log_prob"].detach().numpy().copy(), advantage=loc["advantage"].detach().numpy().copy(),
                           sample=loc["sample"].detach().numpy().copy(), top_lp=float(lp.max(0).values.min()))

    np.random.seed(c["seed"] + 3)
    torch.normal, model.random_elite_idxs = fed_normal, rec_idxs
    grads, worst_lp = [], np.inf
    try:
        obs = None
        for t in range(c["steps"]):
            d = step_inputs(c, t)
            if obs is not None:
                d["obs"] = obs
            queue.append(torch.from_numpy(d["eps"]))
            sys.setprofile(prof)
            try:
                nxt, term, info = pol.dynamics_step_and_forward(d["obs"], d["act"], *(torch.from_numpy(d[k]) for k in
                                                                                  ("sl_obs", "sl_act", "sl_next_obs", "sl_rew")))
            finally:
                sys.setprofile(None)
            assert not queue and len(picked) == t + 1
            tag = f"step{t}"
            if full:
                for k, v in d.items():
                    out[f"{tag}/{k}"] = v
            out[f"{tag}/model_idx"] = picked[t].astype(np.int64)
            out[f"{tag}/losses"] = np.array([info["adv_dynamics_update/" + k] for k in LOSS_KEYS], np.float64)
            out[f"{tag}/log_prob"] = grabbed["log_prob"].reshape(-1)
            out[f"{tag}/advantage"] = grabbed["advantage"].reshape(-1)
            out[f"{tag}/next_obs"], out[f"{tag}/reward"] = nxt, grabbed["sample"][:, -1]
            assert np.array_equal(nxt, grabbed["sample"][:, :-1])
            worst_lp = min(worst_lp, grabbed["top_lp"])
            mk.put_state(out, tag, mk.state(model), full)
            g = {k: p.grad.detach().numpy().copy() for k, p in model.named_parameters() if p.grad is not None}
            grads.append(g)
            out[f"{tag}/grad_max_logvar"], out[f"{tag}/grad_min_logvar"] = g["max_logvar"], g["min_logvar"]
            if full:
                for k, p in model.named_parameters():
                    if p in adv_optim.state:
                        out[f"{tag}/exp_avg/{k}"] = adv_optim.state[p]["exp_avg"].numpy().copy()
                        out[f"{tag}/exp_avg_sq/{k}"] = adv_optim.state[p]["exp_avg_sq"].numpy().copy()
                if t == 0:
                    for k, v in g.items():
                        out[f"{tag}/grad/{k}"] = v
            obs = nxt.copy()
    finally:
        torch.normal, model.random_elite_idxs = orig_normal, orig_idxs
    return out, grads, worst_lp


def gen_tiny(ns, path):
    c = TINY
    w1, g1, lp1 = run_steps(ns, c, 1.0, True)
    w0, g0, lp0 = run_steps(ns, c, 0.0, True)
    # step 0 of both trajectories starts from the same state and rows: the difference of the gradients is the adversarial part
    sl = max(np.abs(v).max() for v in g0[0].values())
    adv = max(np.abs(g1[0][k] - g0[0][k]).max() for k in g0[0])
    print("tiny: adversarial / supervised gradient (max-norm)", adv / sl, "smallest top elite lp_k", min(lp1, lp0))
    assert adv >= 0.3 * sl, (adv, sl)
    assert min(lp1, lp0) > -600, (lp1, lp0)
    ne = [k for k in range(c["K"]) if k not in c["elite_idx"]][0]
    d = g1[0]["output_layer.weight"][ne] - g0[0]["output_layer.weight"][ne]
    assert np.abs(d).max() == 0 and np.abs(g0[0]["output_layer.weight"][ne]).max() > 0      # no elite: supervised gradient only
    out = {("w1/" + k if k.startswith("step") else k): v for k, v in w1.items()}
    out.update({"w0/" + k: v for k, v in w0.items() if k.startswith("step")})
    np.savez_compressed(path, **out)


def gen_mopo(ns, path):
    c = MOPO
    out, _, lp = run_steps(ns, c, c["adv_weight"], False)
    assert lp > -600, lp
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("OFFLINERLKIT_REF", "")
    ns = import_reference(root)
    torch.set_num_threads(4)
    gen_tiny(ns, os.path.join(HERE, "rambo_tiny.npz"))
    gen_mopo(ns, os.path.join(HERE, "rambo_mopo.npz"))
    for f in ("rambo_tiny.npz", "rambo_mopo.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)))

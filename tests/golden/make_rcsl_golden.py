#!/usr/bin/env python3
"""Golden vectors for RCSL from the REAL reference, run on the CPU.  Usage: make_rcsl_golden.py <reference root>.

``RcslPolicy`` (policy/rcsl/rcsl.py), ``RcslModule`` (modules/rcsl_module.py), ``MLP``, ``RcslPolicyTrainer``
(policy_trainer/rcsl_policy_trainer.py), ``DictDataset`` and ``traj_rtg_datasets`` are loaded from the reference tree as they are, the way
make_rambo_golden.import_reference loads the policy side; stubbed: ``offlinerlkit.policy.DiffusionBC`` / ``RcslGaussianPolicy``, ``gym``,
``gymnasium``, ``d4rl``.

Fixtures (inputs are regenerated from rcsl_cases.py, only the reference's outputs are stored):
  rcsl_tiny / rcsl_odd / rcsl_hopper .npz   4 ``learn`` steps: the loss per step, ``pred`` at step 0, the parameter gradient at step 0
                                             (tiny cases), post-step parameters (full for the tiny cases, digests for hopper), the
                                             state_dict key inventory
  rcsl_trainer_trace.npz                     rows / return value / batch order of the real trainer on rcsl_cases' fakes
  rcsl_dataset.npz                           the real ``traj_rtg_datasets`` on rcsl_cases.traj_source()
The script also asserts what the tests rely on: the numpy oracle (tests/rcsl_oracle.py) meets HALF the GPU tests' parameter bar against
the reference, and the tail batch of the ordered-epoch case has a loss that differs from the loss over its rows padded with dataset
row 0 by more than 1e-3 relative (otherwise the masking test would prove nothing)."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
import synth  # noqa: E402
import rcsl_cases as rc  # noqa: E402
import make_rambo_golden as mr  # noqa: E402


def import_reference(root):
    ns = mr.import_reference(root)
    pol = sys.modules["offlinerlkit.policy"]
    pol.DiffusionBC = type("DiffusionBC", (), {})
    for n in ("gymnasium", "d4rl"):
        sys.modules[n] = types.ModuleType(n)
        sys.modules[n].Env = object
    ns.RcslPolicy = importlib.import_module("offlinerlkit.policy.rcsl.rcsl").RcslPolicy
    ns.RcslModule = importlib.import_module("offlinerlkit.modules.rcsl_module").RcslModule
    pol.RcslPolicy, pol.RcslGaussianPolicy = ns.RcslPolicy, type("RcslGaussianPolicy", (), {})
    # packages whose __init__ would pull in the rest of the tree: shells that load submodules from the tree
    for pkg in ("policy_trainer", "buffer"):
        m = types.ModuleType("offlinerlkit." + pkg)
        m.__path__ = [os.path.join(root, "offlinerlkit", pkg)]
        sys.modules["offlinerlkit." + pkg] = m
    sys.modules["offlinerlkit.buffer"].ReplayBuffer = object
    sys.modules["offlinerlkit.utils"].__path__ = [os.path.join(root, "offlinerlkit", "utils")]
    ns.Trainer = importlib.import_module("offlinerlkit.policy_trainer.rcsl_policy_trainer").RcslPolicyTrainer
    ns.load_dataset = importlib.import_module("offlinerlkit.utils.load_dataset")
    return ns


def build(ns, c, net):
    bb = ns.MLP(input_dim=c["obs_dim"] + 1, hidden_dims=c["hidden"], output_dim=c["act_dim"])
    mod = ns.RcslModule(bb, "cpu")
    with torch.no_grad():
        for k, p in mod.named_parameters():
            p.copy_(torch.from_numpy(net[k]))
    return ns.RcslPolicy(None, None, mod, torch.optim.Adam(mod.parameters(), lr=c["lr"]), "cpu")


def tbatch(b):
    return {k: torch.from_numpy(v) for k, v in b.items()}


def learn_fixture(ns, case):
    import rcsl_oracle as orc
    c, net, batches = rc.case_inputs(case)
    pol = build(ns, c, net)
    st = orc.init_state(net)
    out = {"loss_keys": np.array(["loss"]), "keys": np.array(list(pol.state_dict().keys()))}
    scale = c["lr"] / 3e-4
    for k, b in enumerate(batches):
        if k == 0:
            with torch.no_grad():
                out["step0/pred"] = pol.rcsl(b["observations"], b["rtgs"]).numpy().copy()
            # the gradient learn() is about to apply (learn zeroes it before its own backward)
            loss = torch.pow(pol.rcsl(b["observations"], b["rtgs"]) - torch.from_numpy(b["actions"]), 2).mean()
            pol.rcsl_optim.zero_grad(); loss.backward()
            if c["full"]:
                for n, p in pol.rcsl.named_parameters():
                    out[f"step0/grads/{n}"] = p.grad.numpy().copy()
        res = pol.learn(tbatch(b))
        assert list(res.keys()) == ["loss"]
        out[f"step{k}/losses"] = np.array([res["loss"]], np.float64)
        ores, _ = orc.learn(st, c, b)
        assert abs(ores["loss"] - res["loss"]) <= 1e-4 * max(abs(res["loss"]), 1e-2 * abs(res["loss"])), (case, k, ores, res)
        for n, p in pol.rcsl.named_parameters():
            v = p.detach().numpy().copy()
            out[f"state{k}/rcsl/{n}/digest"] = synth.digest(v)
            if c["full"]:
                out[f"state{k}/rcsl/{n}/full"] = v
            # the oracle against the reference at HALF the GPU tests' bar (tests/test_gpu_rcsl.py: 4e-6 (k + 1) lr / 3e-4 + 1e-4 max |p|)
            d = np.abs(st["rcsl"][n] - v)
            assert d.max() <= 2e-6 * (k + 1) * scale + 0.5e-4 * np.abs(v).max(), (case, k, n, d.max())
            assert d.mean() < 0.5e-6 * (k + 1) * scale, (case, k, n, d.mean())
    np.savez_compressed(os.path.join(HERE, case + ".npz"), **out)
    print(case, [float(out[f"step{k}/losses"][0]) for k in range(rc.STEPS)])


def vacuity(ns):
    """the ordered-epoch case: the tail step's loss over its 5 valid rows vs over all B gathered rows (padding reads dataset row 0)"""
    c, data, orders = rc.epoch_inputs("rcsl_tiny")
    _, net, _ = rc.case_inputs("rcsl_tiny")
    B = c["B"]
    for r in range(orders[0].shape[0]):
        idx = orders[0][r, 3 * B:]
        assert (idx >= 0).sum() == 5
        pol = build(ns, c, net)
        tail = pol.learn(tbatch(rc.gather(data, idx[idx >= 0])))["loss"]
        pol = build(ns, c, net)
        padded = pol.learn(tbatch(rc.gather(data, idx)))["loss"]
        assert abs(tail - padded) > 1e-3 * abs(tail), (r, tail, padded)
        print("tail vs padded loss, run", r, tail, padded)


def trainer_fixture(ns):
    out = {}
    for v in rc.TRAINER_VARIANTS:
        for k, a in rc.run_trainer(ns.Trainer, v).items():
            out[f"{v}/{k}"] = a
        print(v, list(out[f"{v}/keys"]), out[f"{v}/last_10"])
    np.savez_compressed(os.path.join(HERE, "rcsl_trainer_trace.npz"), **out)


def dataset_fixture(ns):
    out = {}
    for tag, use_to in (("timeouts", True), ("steps", False)):
        full, init_obss, max_ret = ns.load_dataset.traj_rtg_datasets(rc.TrajEnv(use_to))
        for k, v in full.items():
            out[f"{tag}/{k}"] = v
        out[f"{tag}/init_obss"], out[f"{tag}/max_return"] = init_obss, np.array([max_ret])
        print(tag, {k: v.shape for k, v in full.items()}, init_obss.shape, max_ret)
    np.savez_compressed(os.path.join(HERE, "rcsl_dataset.npz"), **out)


def main():
    root = sys.argv[1]
    sys.path.insert(0, root)
    ns = import_reference(root)
    torch.set_num_threads(1)
    for case in rc.CASES:
        learn_fixture(ns, case)
    vacuity(ns)
    dataset_fixture(ns)
    trainer_fixture(ns)


if __name__ == "__main__":
    main()

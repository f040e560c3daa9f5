#!/usr/bin/env python3
"""Golden vectors for Gaussian RCSL from the REAL reference, run on the CPU.  Usage: make_rcsl_gauss_golden.py <reference root> [--search].

``RcslGaussianPolicy`` (policy/rcsl/rcsl_gauss.py), ``RcslGaussianModule`` (modules/rcsl_gauss_module.py), ``DiagGaussian``
(modules/dist_module.py) and ``MLP`` are loaded from the reference tree as they are, on top of make_rcsl_golden.import_reference.

Fixtures (inputs are regenerated from rcsl_gauss_cases.py, only the reference's outputs are stored): rcslg_<case>.npz with 4 ``learn``
steps: the loss per step, ``mu`` / ``logvar`` of ``get_dist_params`` at step 0, the parameter gradient at step 0 (full cases), post-step
parameters (full for the small cases, digests for the large ones), the state_dict key inventory.
The script also asserts what the tests rely on:
  * the clamp conditions of rcsl_gauss_cases.py's docstring at every step in the reference ("clamp" heads: both bounds active, a margin of
    1e-3 of the scale around each; "open" heads: every value at least 1 inside); ``--search`` prints the head seed offsets that meet them;
  * the numpy oracle (tests/rcsl_gauss_oracle.py) meets HALF the GPU tests' parameter bar against the reference, head tensors included,
    and the distances are printed;
  * the tail batch of the ordered-epoch case has a loss that differs from the loss over its rows padded with dataset row 0 by more than
    1e-3 relative (otherwise the masking test would prove nothing)."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
import synth  # noqa: E402
import rcsl_cases as rc  # noqa: E402
import rcsl_gauss_cases as gc  # noqa: E402
import make_rcsl_golden as mg  # noqa: E402


def import_reference(root):
    ns = mg.import_reference(root)
    ns.DiagGaussian = importlib.import_module("offlinerlkit.modules.dist_module").DiagGaussian
    ns.RcslGaussianModule = importlib.import_module("offlinerlkit.modules.rcsl_gauss_module").RcslGaussianModule
    ns.RcslGaussianPolicy = importlib.import_module("offlinerlkit.policy.rcsl.rcsl_gauss").RcslGaussianPolicy
    return ns


def build(ns, c, net):
    A = c["act_dim"]
    bb = ns.MLP(input_dim=c["obs_dim"] + 1, hidden_dims=c["hidden"], output_dim=A)
    mod = ns.RcslGaussianModule(bb, ns.DiagGaussian(latent_dim=A, output_dim=A, unbounded=True, conditioned_sigma=True), "cpu")
    with torch.no_grad():
        for k, p in mod.named_parameters():
            p.copy_(torch.from_numpy(net[k]))
    return ns.RcslGaussianPolicy(None, None, mod, torch.optim.Adam(mod.parameters(), lr=c["lr"]), "cpu")


def tbatch(b):
    return {k: torch.from_numpy(v) for k, v in b.items()}


def raw_sigma(pol, b):
    """the sigma head before its clamp, from the reference's own modules"""
    with torch.no_grad():
        rtg = torch.from_numpy(b["rtgs"])
        z = pol.rcsl.backbone(torch.cat([torch.from_numpy(b["observations"]), rtg], dim=-1))
        return pol.rcsl.dist_net.sigma(z).numpy()


def clamp_report(c, raw):
    """(fraction clamped low, high, margin to the nearer bound over max |raw|)"""
    lo, hi = float((raw < gc.LO).mean()), float((raw > gc.HI).mean())
    margin = float(min(np.abs(raw - gc.LO).min(), np.abs(raw - gc.HI).min()) / np.abs(raw).max())
    return lo, hi, margin


def clamp_ok(c, raw):
    if c["head"] == "open":
        return bool((raw >= gc.LO + 1.0).all() and (raw <= gc.HI - 1.0).all())
    lo, hi, margin = clamp_report(c, raw)
    return lo >= 0.03 and hi >= 0.03 and lo + hi <= 0.75 and margin >= 1e-3


def search(ns, case, n=120):
    good = []
    for off in range(n):
        c, net, batches = gc.case_inputs(case, offset=off)
        pol = build(ns, c, net)
        ok, worst = True, 1.0
        for b in batches:
            raw = raw_sigma(pol, b)
            ok = ok and clamp_ok(c, raw)
            worst = min(worst, clamp_report(c, raw)[2])
            if not ok:
                break
            pol.learn(tbatch(b))
        if ok:
            good.append((off, worst))
    print(case, "head seed offsets that meet the clamp conditions (offset, margin / scale):", good)


def learn_fixture(ns, case):
    import rcsl_gauss_oracle as orc
    c, net, batches = gc.case_inputs(case)
    pol = build(ns, c, net)
    st = orc.init_state(net)
    out = {"loss_keys": np.array(["loss"]), "keys": np.array(list(pol.state_dict().keys()))}
    scale = c["lr"] / 3e-4
    worst_abs, worst_mean, clamps = 0.0, 0.0, []
    for k, b in enumerate(batches):
        raw = raw_sigma(pol, b)
        assert clamp_ok(c, raw), (case, k, clamp_report(c, raw))
        clamps.append(clamp_report(c, raw))
        if k == 0:
            with torch.no_grad():
                mu, logvar = pol.rcsl.get_dist_params(b["observations"], b["rtgs"])
                out["step0/mu"], out["step0/logvar"] = mu.numpy().copy(), logvar.numpy().copy()
            # the gradient learn() is about to apply (learn zeroes it before its own backward)
            mu, logvar = pol.rcsl.get_dist_params(b["observations"], b["rtgs"])
            loss = (torch.pow(mu - torch.from_numpy(b["actions"]), 2) * torch.exp(-logvar)).mean() + logvar.mean()
            pol.rcsl_optim.zero_grad(); loss.backward()
            if c["full"]:
                for n, p in pol.rcsl.named_parameters():
                    out[f"step0/grads/{n}"] = p.grad.numpy().copy()
        res = pol.learn(tbatch(b))
        assert list(res.keys()) == ["loss"]
        out[f"step{k}/losses"] = np.array([res["loss"]], np.float64)
        ores, aux = orc.learn(st, c, b)
        assert abs(ores["loss"] - res["loss"]) <= 1e-4 * max(abs(res["loss"]), 1e-2 * abs(res["loss"])), (case, k, ores, res)
        if k == 0:
            for nm in ("mu", "logvar"):
                assert np.abs(aux[nm] - out[f"step0/{nm}"]).max() <= 1e-5 * np.abs(out[f"step0/{nm}"]).max(), (case, nm)
        for n, p in pol.rcsl.named_parameters():
            v = p.detach().numpy().copy()
            out[f"state{k}/rcsl/{n}/digest"] = synth.digest(v)
            if c["full"]:
                out[f"state{k}/rcsl/{n}/full"] = v
            # the oracle against the reference at HALF the GPU tests' bar (tests/test_gpu_rcsl.py: 4e-6 (k + 1) lr / 3e-4 + 1e-4 max |p|)
            d = np.abs(st["rcsl"][n] - v)
            assert d.max() <= 2e-6 * (k + 1) * scale + 0.5e-4 * np.abs(v).max(), (case, k, n, d.max())
            assert d.mean() < 0.5e-6 * (k + 1) * scale, (case, k, n, d.mean())
            worst_abs, worst_mean = max(worst_abs, d.max() / ((k + 1) * scale)), max(worst_mean, d.mean() / ((k + 1) * scale))
    np.savez_compressed(os.path.join(HERE, case + ".npz"), **out)
    print(case, [float(out[f"step{k}/losses"][0]) for k in range(gc.STEPS)])
    print("   clamped low / high / margin per step:", [tuple(round(x, 4) for x in cl) for cl in clamps])
    print(f"   oracle vs reference parameters, over (k + 1) lr / 3e-4: max {worst_abs:.2e} (bar 2e-6 + rel), mean {worst_mean:.2e} (bar 5e-7)")


def vacuity(ns):
    """the ordered-epoch case: the tail step's loss over its 5 valid rows vs over all B gathered rows (padding reads dataset row 0)"""
    c, data, orders = gc.epoch_inputs()
    _, net, _ = gc.case_inputs("rcslg_tiny")
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


def main():
    root = sys.argv[1]
    sys.path.insert(0, root)
    ns = import_reference(root)
    torch.set_num_threads(1)
    if "--search" in sys.argv:
        for case, c in gc.CASES.items():
            if c["head"] == "clamp":
                search(ns, case)
        return
    for case in gc.CASES:
        learn_fixture(ns, case)
    vacuity(ns)


if __name__ == "__main__":
    main()

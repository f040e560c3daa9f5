#!/usr/bin/env python3
"""Golden vectors for the autoregressive behaviour policy and for ``RcslPolicy.rollout`` from the REAL reference, run on the CPU.
Usage: make_autoreg_golden.py <reference root> [--search].

``AutoregressivePolicy`` is loaded from the reference's policy/others/autoregressive.py as it is (it needs only torch); ``RcslPolicy``
(for ``rollout``) through make_rcsl_golden.import_reference.

Fixtures (inputs are regenerated from autoreg_cases.py, only the reference's outputs are stored):
  ar_<case>.npz        4 ``learn`` steps: the loss per step, ``mean`` / ``logstd`` of the expanded rows at step 0, the parameter gradient at
                       step 0 (full cases and ar_ws), post-step parameters (full for the small cases, digests for the large ones), the
                       state_dict key inventory
  ar_sample.npz        for ar_tiny / ar_odd / ar_act32 and 8 rows each: the ``eps`` the generator drew (torch.randn(1, 1) per dimension
                       after torch.manual_seed(seed0 + row), what Normal.sample consumes) and the reference's one-row ``select_action``
                       under the same seed
  ar_rollout.npz       the reference's ``RcslPolicy.rollout`` on autoreg_cases' fake dynamics and rollout policies: every output array and
                       info value.  For the policy without ``sample_init_noise`` the reference's own call is stubbed HERE only (a
                       ``sample_init_noise`` that returns an index array, a ``select_action`` that drops it)
The script also asserts what the tests rely on, and prints the measured distances:
  * both signs at the output: at every step in the reference at least 10 % of the tail pre-activations lie on each side of zero in each
    of the two columns and none within 1e-3 of max |z_tail| of zero (``--search`` prints the output-layer seed offsets that meet it);
    ar_hopper at step 0 only, its later steps are printed (autoreg_cases.py says why);
  * both signs in the hidden layers: every hidden layer has both signs in at least 10 % of its units;
  * the numpy oracle (tests/autoreg_oracle.py) meets HALF the GPU tests' parameter bar against the reference;
  * the tail batch of the ordered-epoch case has a loss that differs from the loss over all B gathered rows by more than 1e-3 relative;
  * the oracle fed the stored ``eps`` reproduces the reference's sampled action to 1e-6 of its scale."""
import importlib.util
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
import autoreg_cases as ac  # noqa: E402
import autoreg_oracle as orc  # noqa: E402


def load_policy_class(root):
    spec = importlib.util.spec_from_file_location("ref_autoregressive", os.path.join(root, "offlinerlkit", "policy", "others", "autoregressive.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.AutoregressivePolicy


def build(Policy, c, net):
    pol = Policy(c["obs_dim"], c["act_dim"], list(c["hidden"]), c["lr"], "cpu")
    with torch.no_grad():
        for k, p in pol.named_parameters():
            p.copy_(torch.from_numpy(net[k]))
    return pol


def tbatch(b):
    return {k: torch.from_numpy(v) for k, v in b.items()}


def pre_activations(pol, b):
    """the pre-activations of every Linear on the expanded rows of ``fit``, from the reference's own modules"""
    x, _ = orc.expand(b["observations"], b["actions"])
    zs = []
    with torch.no_grad():
        h = torch.from_numpy(x)
        for layer in pol.model:
            h = layer(h)
            if isinstance(layer, torch.nn.Linear):
                zs.append(h.numpy().copy())
    return zs


def sign_report(zs):
    """(smallest share of a side over the two output columns, margin to zero / max |z_tail|, smallest share of units with both signs over the hidden layers)"""
    zt = zs[-1]
    side = min(min(float((zt[:, c] > 0).mean()), float((zt[:, c] < 0).mean())) for c in range(2))
    margin = float(np.abs(zt).min() / np.abs(zt).max())
    both = min((float(((z > 0).any(axis=0) & (z < 0).any(axis=0)).mean()) for z in zs[:-1]), default=1.0)
    return side, margin, both


def signs_ok(rep):
    return rep[0] >= 0.10 and rep[1] >= 1e-3 and rep[2] >= 0.10


def search(Policy, case, n=400):
    good = []
    for off in range(n):
        c, net, batches = ac.case_inputs(case, offset=off)
        pol = build(Policy, c, net)
        ok, worst = True, (1.0, 1.0, 1.0)
        for b in batches[:c.get("sign_steps", ac.STEPS)]:
            rep = sign_report(pre_activations(pol, b))
            worst = tuple(min(a, x) for a, x in zip(worst, rep))
            ok = signs_ok(rep)
            if not ok:
                break
            pol.learn(tbatch(b))
        if ok:
            good.append((off, tuple(round(x, 4) for x in worst)))
    print(case, "output-layer seed offsets that meet the sign conditions (offset, (side share, margin / scale, hidden share)):", good[:12])


def learn_fixture(Policy, case):
    c, net, batches = ac.case_inputs(case)
    pol = build(Policy, c, net)
    st = orc.init_state(net)
    out = {"loss_keys": np.array(["loss"]), "keys": np.array(list(pol.state_dict().keys()))}
    scale = c["lr"] / 3e-4
    worst_abs, worst_mean, signs = 0.0, 0.0, []
    for k, b in enumerate(batches):
        rep = sign_report(pre_activations(pol, b))
        assert signs_ok(rep) or k >= c.get("sign_steps", ac.STEPS), (case, k, rep)
        signs.append(rep)
        if k == 0:
            with torch.no_grad():
                h = torch.from_numpy(orc.expand(b["observations"], b["actions"])[0])
                for layer in pol.model:
                    h = layer(h)
                out["step0/mean"], out["step0/logstd"] = h[:, 0].numpy().copy(), h[:, 1].numpy().copy()
            # the gradient learn() is about to apply (learn zeroes it before its own backward)
            loss = pol.fit(torch.from_numpy(b["observations"]), torch.from_numpy(b["actions"]))
            pol.rcsl_optim.zero_grad(); loss.backward()
            if c["full"] or c.get("grads"):
                for n, p in pol.named_parameters():
                    out[f"step0/grads/{n}"] = p.grad.numpy().copy()
        res = pol.learn(tbatch(b))
        assert list(res.keys()) == ["loss"]
        out[f"step{k}/losses"] = np.array([res["loss"]], np.float64)
        ores, aux = orc.learn(st, c, b)
        assert abs(ores["loss"] - res["loss"]) <= 1e-4 * max(abs(res["loss"]), 1e-2), (case, k, ores, res)
        if k == 0:
            for nm in ("mean", "logstd"):
                assert np.abs(aux[nm] - out[f"step0/{nm}"]).max() <= 1e-5 * np.abs(out[f"step0/{nm}"]).max(), (case, nm)
        for n, p in pol.named_parameters():
            v = p.detach().numpy().copy()
            out[f"state{k}/model/{n}/digest"] = synth.digest(v)
            if c["full"]:
                out[f"state{k}/model/{n}/full"] = v
            # the oracle against the reference at HALF the GPU tests' bar (tests/test_gpu_rcsl.py: 4e-6 (k + 1) lr / 3e-4 + 1e-4 max |p|)
            d = np.abs(st["model"][n] - v)
            assert d.max() <= 2e-6 * (k + 1) * scale + 0.5e-4 * np.abs(v).max(), (case, k, n, d.max())
            assert d.mean() < 0.5e-6 * (k + 1) * scale, (case, k, n, d.mean())
            worst_abs, worst_mean = max(worst_abs, d.max() / ((k + 1) * scale)), max(worst_mean, d.mean() / ((k + 1) * scale))
    np.savez_compressed(os.path.join(HERE, case + ".npz"), **out)
    print(case, [float(out[f"step{k}/losses"][0]) for k in range(ac.STEPS)])
    print("   side share / margin / hidden share per step:", [tuple(round(x, 4) for x in s) for s in signs])
    print(f"   oracle vs reference parameters, over (k + 1) lr / 3e-4: max {worst_abs:.2e} (bar 2e-6 + rel), mean {worst_mean:.2e} (bar 5e-7)")


def vacuity(Policy):
    """the ordered-epoch case: the tail step's loss over its 5 valid rows vs over all B gathered rows (padding reads dataset row 0)"""
    c, data, orders = ac.epoch_inputs()
    _, net, _ = ac.case_inputs("ar_tiny")
    B = c["B"]
    for r in range(orders[0].shape[0]):
        idx = orders[0][r, 3 * B:]
        assert (idx >= 0).sum() == 5
        tail = build(Policy, c, net).learn(tbatch(ac.gather(data, idx[idx >= 0])))["loss"]
        padded = build(Policy, c, net).learn(tbatch(ac.gather(data, idx)))["loss"]
        assert abs(tail - padded) > 1e-3 * abs(tail), (r, tail, padded)
        print("tail vs padded loss, run", r, tail, padded)


def sample_fixture(Policy):
    out = {}
    for case in ac.SAMPLE_CASES:
        c, net, _ = ac.case_inputs(case)
        pol = build(Policy, c, net)
        obs = ac.sample_obs(case)
        A = c["act_dim"]
        eps, acts = np.zeros((ac.SAMPLE_ROWS, A), np.float32), np.zeros((ac.SAMPLE_ROWS, A), np.float32)
        for i in range(ac.SAMPLE_ROWS):
            torch.manual_seed(ac.SAMPLE_SEED0 + i)
            eps[i] = [float(torch.randn(1, 1)) for _ in range(A)]
            torch.manual_seed(ac.SAMPLE_SEED0 + i)
            acts[i] = pol.select_action(obs[i:i + 1], None)[0]
        want = orc.sample(net, obs, eps)
        err = np.abs(want - acts).max() / np.abs(acts).max()
        assert err <= 1e-6, (case, err)      # (which proves the stored eps is what the reference consumed)
        out[f"{case}/eps"], out[f"{case}/actions"] = eps, acts
        print(f"{case}: oracle fed the stored eps vs the reference's select_action: {err:.2e} of scale")
    np.savez_compressed(os.path.join(HERE, "ar_sample.npz"), **out)


def rollout_fixture(root):
    import make_rcsl_golden as mg
    ns = mg.import_reference(root)
    out = {}
    for name in ac.ROLLOUTS:
        dyn, rp, init, horizon = ac.rollout_collaborators(name)
        if not hasattr(rp, "sample_init_noise"):
            class Stub:      # the reference calls sample_init_noise unconditionally and indexes the result: give it something to index
                def sample_init_noise(self, n):
                    return np.zeros((n, 1), np.float32)

                def select_action(self, obs, noise):
                    return rp.select_action(obs, None)
            use = Stub()
        else:
            use = rp
        pol = ns.RcslPolicy(dyn, use, torch.nn.Linear(1, 1), None, "cpu")
        tr, info = pol.rollout(init, horizon)
        for k, v in tr.items():
            out[f"{name}/{k}"] = np.asarray(v)
        out[f"{name}/info/num_transitions"] = np.array([info["num_transitions"]], np.int64)
        out[f"{name}/info/reward_mean"] = np.array([info["reward_mean"]], np.float64)
        out[f"{name}/info/returns"] = np.asarray(info["returns"], np.float64)
        print(name, {k: np.asarray(v).shape for k, v in tr.items()}, info["num_transitions"], float(info["reward_mean"]))
    assert out["all_end_early/obss"].shape[0] < 7 * 9 and out["all_end_early/terminals"][-1].all()
    np.savez_compressed(os.path.join(HERE, "ar_rollout.npz"), **out)


def main():
    root = sys.argv[1]
    Policy = load_policy_class(root)
    torch.set_num_threads(1)
    if "--search" in sys.argv:
        for case in sys.argv[3:] or ac.CASES:
            search(Policy, case)
        return
    for case in ac.CASES:
        learn_fixture(Policy, case)
    vacuity(Policy)
    sample_fixture(Policy)
    sys.path.insert(0, root)
    rollout_fixture(root)


if __name__ == "__main__":
    main()

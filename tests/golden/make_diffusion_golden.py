#!/usr/bin/env python3
"""Golden vectors for DiffusionBC from the REAL reference net, run on the CPU.  Usage: make_diffusion_golden.py <reference root>.

The reference's own code: ``ConditionalUnet1D`` (offlinerlkit/nets/unet.py), imported from the reference tree as it is and called the
way policy/others/diffusion.py calls it (``action.unsqueeze(1)``, a per-row timestep tensor, ``global_cond=obs``), torch's
``mse_loss``, autograd, ``torch.optim.AdamW(lr=1e-4, weight_decay=1e-6)``.  (The float64 gradients of (a) alone come from the project's own
``offlinerlkit.nets.ConditionalUnet1D`` -- the reference's forward casts to float32 inside --, which tests/test_diffusion_cpu.py holds
bit for bit to this fixture in float32.)
Restated here, because ``diffusers`` is not available: the DDPM scheduler (squared-cosine betas, ``add_noise``, the clipped epsilon
step with ``fixed_small`` variance), the cosine learning-rate schedule with 500 warm-up steps (set on the optimizer before every step)
and the EMA of power 0.75 -- the formulas of DESIGN.md, which the engine and tests/diffusion_oracle.py restate independently.
Inputs come from diffusion_cases.py; only the reference's outputs are stored.

Fixtures:
  diffusion_a.npz   down_dims [8, 16, 32] (70 883 parameters; group sizes 1, 2, 4), one batch of 6: pred, loss, x_t, the gradient of
                    every parameter (off-centre conv taps included: exactly zero), and ``grad_f32_vs_f64``
  diffusion_b.npz   down_dims [8, 16] (20 659 parameters): 20 teacher-forced steps (10 epochs of 6 + 2 rows): losses, final parameters,
                    final EMA; the same for the twin whose initial parameters are moved by one ulp
  diffusion_c.npz   the net of (b): ``select_action`` for 4 rows with given init_noise and z
  diffusion_d.npz   down_dims [24, 32] (83 811 parameters; groups of 3 and 4 channels, none of 1: every tensor has a gradient and the
                    output depends on every block): for the batch of 6 and the short one of 2: pred, loss, x_t, the float64 gradient of
                    every tensor (conv weights as their centre tap; stored rounded to float32) and ``grad_f32_vs_f64`` of that
                    batch; ``select_action`` for 4 rows
  diffusion_e.npz   down_dims [16, 32] with n_groups = 4: the blocks normalise groups of 4 and 8 channels, final_conv keeps GroupNorm(8)
                    (its Conv1dBlock is built without n_groups); one batch of 6: pred, loss, x_t, float64 gradients, ``grad_f32_vs_f64``
  diffusion_d_traj.npz  the same net as (d): 12 teacher-forced steps (6 epochs of 6 + 2 rows): losses, final parameters and EMA (centre taps),
                    and the one-ulp twin's
The script asserts what the tests rely on and prints the measured distances:
  * the off-centre taps' gradient is exactly zero, and AdamW's parameters equal Adam's bit for bit after the 20 steps;
  * fp32 autograd against float64 autograd on fixture (a), per tensor max |g32 - g64| / max |g64|: measured 3.4e-05 on the worst of the
    THREE tensors that have a gradient.  final_conv's GroupNorm(8) over 8 channels has one channel per group: its output is its beta
    whatever it reads, so in (a) -- and in (b) -- only final_conv.0's beta and final_conv.1 receive a gradient and every other tensor's
    is structurally zero (float64: <= 1e-14); fp32 autograd leaves cancellation noise of up to 3.2e-05 there.  Both numbers are stored;
    the GPU test gives the engine 4 times each.  Fixture (d) is the same measurement on a net without such a norm: per tensor
    max |g32 - g64| / max |g64|, worst tensor, 7.1e-06 on the batch of 6 and 1.7e-05 on the batch of 2; the engine, the numpy oracle
    and the project's torch module get 4 times the stored value of the batch;
  * the numpy oracle reproduces pred / loss / gradients of (a) and the trajectory of (b) and the actions of (c)."""
import contextlib
import importlib.util
import io
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
import diffusion_cases as dc  # noqa: E402
import diffusion_oracle as orc  # noqa: E402
from diffusion_oracle import grad_distance  # noqa: E402


def load_unet(root):
    spec = importlib.util.spec_from_file_location("ref_unet", os.path.join(root, "offlinerlkit", "nets", "unet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ConditionalUnet1D


def build(Unet, c, params=None, dtype=torch.float32):
    with contextlib.redirect_stdout(io.StringIO()):
        net = Unet(input_dim=c["act_dim"], global_cond_dim=c["obs_dim"], **dc.net_kwargs(c))
    if params is None:
        params = dc.make_params(c, [(k, tuple(v.shape)) for k, v in net.state_dict().items()])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return net.to(dtype), params


def centre(v):
    """a conv weight's centre tap [out, in] (the other taps never change and have no gradient); any other tensor as it is"""
    return v[:, :, v.shape[2] // 2] if v.ndim == 3 else v


def batch_loss(net, c, act, t, eps, obs, dtype=torch.float32):
    acp = torch.from_numpy(orc.alphas_cumprod(c["N"]))
    tt = torch.from_numpy(t)
    action = torch.from_numpy(act).unsqueeze(1)
    noise = torch.from_numpy(eps).unsqueeze(1)
    sa, sb = (acp[tt] ** 0.5).reshape(-1, 1, 1), ((1 - acp[tt]) ** 0.5).reshape(-1, 1, 1)
    noisy = (sa * action + sb * noise).type(torch.float32)
    pred = net(noisy.to(dtype), tt, global_cond=torch.from_numpy(obs).to(dtype))
    return torch.nn.functional.mse_loss(pred, noise.to(dtype)), pred, noisy


def run_training(Unet, c, params, steps, total, opt_cls=torch.optim.AdamW):
    net, _ = build(Unet, c, params)
    obs, act = dc.make_data(c)
    kw = dict(weight_decay=1e-6) if opt_cls is torch.optim.AdamW else {}
    opt = opt_cls(net.parameters(), lr=1e-4, **kw)
    ema = {k: v.detach().clone() for k, v in net.named_parameters()}
    losses = []
    for k, (idx, t, eps) in enumerate(steps):
        for gparam in opt.param_groups:
            gparam["lr"] = orc.lr_at(k, total)
        loss, _, _ = batch_loss(net, c, act[idx], t, eps, obs[idx])
        opt.zero_grad()
        loss.backward()
        opt.step()
        d = orc.ema_decay(k)
        with torch.no_grad():
            for name, p in net.named_parameters():
                ema[name].mul_(d).add_(p, alpha=1 - d)
        losses.append(loss.item())
    return np.array(losses, np.float64), {k: v.detach().numpy().copy() for k, v in net.named_parameters()}, {k: v.numpy().copy() for k, v in ema.items()}


def sample(net, c, obs, init_noise, z):
    acp = torch.from_numpy(orc.alphas_cumprod(c["N"]))
    x = torch.from_numpy(init_noise).clone()
    o = torch.from_numpy(obs)
    one = torch.tensor(1.0)
    with torch.no_grad():
        for t in range(c["N"] - 1, -1, -1):
            e = net(sample=x, timestep=t, global_cond=o)
            a, ap = acp[t], (acp[t - 1] if t > 0 else one)
            at = a / ap
            x0 = ((x - (1 - a) ** 0.5 * e) / a ** 0.5).clamp(-1, 1)
            x = ap ** 0.5 * (1 - at) / (1 - a) * x0 + at ** 0.5 * (1 - ap) / (1 - a) * x
            if t > 0:
                x = x + torch.clamp((1 - ap) / (1 - a) * (1 - at), min=1e-20) ** 0.5 * torch.from_numpy(z[t]).unsqueeze(1)
    return x.numpy()[:, 0, :]


def main(root):
    torch.set_num_threads(1)
    Unet = load_unet(root)
    # ---- (a) -------------------------------------------------------------------------------------------------------------------
    c = dc.CASES["a"]
    net, P = build(Unet, c)
    print("(a) parameters:", sum(p.numel() for p in net.parameters()))
    obs, act = dc.make_data(c)
    idx, t, eps = dc.make_steps(c, 1)[0]
    loss, pred, noisy = batch_loss(net, c, act[idx], t, eps, obs[idx])
    loss.backward()
    g32 = {k: p.grad.numpy().copy() for k, p in net.named_parameters()}
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "offlinerl-kit_amd"))
    from offlinerlkit.nets import ConditionalUnet1D as OurUnet      # the reference's forward casts to float32 inside; ours keeps the dtype
    net64, _ = build(OurUnet, c, P, torch.float64)
    loss64, _, _ = batch_loss(net64, c, act[idx], t, eps, obs[idx], torch.float64)
    loss64.backward()
    g64 = {k: p.grad.numpy().copy() for k, p in net64.named_parameters()}
    for k, g in g32.items():
        if g.ndim == 3 and g.shape[2] > 1:
            off = np.delete(g, g.shape[2] // 2, axis=2)
            assert not off.any(), ("off-centre gradient", k)
    dist, noise = grad_distance(g32, g64)
    live = [k for k, v in g64.items() if np.abs(v).max() > 1e-9 * max(np.abs(w).max() for w in g64.values())]
    print(f"(a) fp32 vs float64 autograd, worst tensor: {dist:.3e}; fp32 noise on the structurally zero tensors {noise:.3e}; "
          f"tensors with a gradient: {live}; loss {loss.item():.6f}")
    ol, op, og, oxt = orc.loss_and_grads(P, c, act[idx], t, eps, obs[idx])
    od, on = grad_distance(og, g64)
    print(f"    oracle: pred {np.abs(op - pred.detach().numpy()[:, 0]).max():.2e} loss {abs(ol - loss.item()):.2e} grads {od:.3e} / {on:.3e}")
    assert od < 4 * dist and on <= 4 * noise
    out = {"pred": pred.detach().numpy()[:, 0], "loss": np.float64(loss.item()), "x_t": noisy.numpy()[:, 0],
           "grad_f32_vs_f64": np.float64(dist), "grad_zero_noise": np.float64(noise)}
    out.update({f"grad64/{k}": g64[k] for k in live})
    out.update({f"grad/{k}": v for k, v in g32.items()})
    np.savez_compressed(os.path.join(HERE, "diffusion_a.npz"), **out)
    # ---- (b) -------------------------------------------------------------------------------------------------------------------
    c = dc.CASES["b"]
    _, P = build(Unet, c)
    steps = dc.make_steps(c, c["steps"])
    total = c["steps"]
    losses, fin, ema = run_training(Unet, c, P, steps, total)
    _, fin_adam, _ = run_training(Unet, c, P, steps, total, torch.optim.Adam)
    assert all(np.array_equal(fin[k], fin_adam[k]) for k in fin), "AdamW != Adam"
    for k, v in fin.items():
        if v.ndim == 3 and v.shape[2] > 1:
            assert np.array_equal(np.delete(v, v.shape[2] // 2, axis=2), np.delete(P[k], v.shape[2] // 2, axis=2)), ("off-centre tap moved", k)
    twin = {k: np.nextafter(v, np.float32(np.inf)).astype(np.float32) for k, v in P.items()}
    tl, tfin, tema = run_training(Unet, c, twin, steps, total)
    olosses, ofin, oema = orc.train(P, c, dc.make_data(c), steps, total)
    print(f"(b) losses {losses[0]:.5f} .. {losses[-1]:.5f}; twin max |dloss| {np.abs(tl - losses).max():.2e}; oracle {np.abs(olosses - losses).max():.2e}")
    print(f"    params: twin {max(np.abs(tfin[k] - fin[k]).max() for k in fin):.2e} oracle {max(np.abs(ofin[k] - fin[k]).max() for k in fin):.2e}")
    out = {"losses": losses, "losses_twin": tl}
    for k in fin:
        out[f"final/{k}"], out[f"ema/{k}"], out[f"final_twin/{k}"], out[f"ema_twin/{k}"] = fin[k], ema[k], tfin[k], tema[k]
    np.savez_compressed(os.path.join(HERE, "diffusion_b.npz"), **out)
    # ---- (c) -------------------------------------------------------------------------------------------------------------------
    c = dc.CASES["c"]
    net, P = build(Unet, c)
    obs, noise, z = dc.make_sample_inputs(c)
    a = sample(net, c, obs, noise, z)
    oa = orc.sample(P, c, obs, noise, z)
    print(f"(c) actions\n{a}\n    oracle max |d| {np.abs(oa - a).max():.2e}")
    np.savez_compressed(os.path.join(HERE, "diffusion_c.npz"), actions=a)
    # ---- (d): a net whose every tensor has a gradient, from the reference's own module ------------------------------------------
    c = dc.CASES["d"]
    net, P = build(Unet, c)
    print("(d) parameters:", sum(p.numel() for p in net.parameters()))
    obs, act = dc.make_data(c)
    out = {}
    for b, (idx, t, eps) in enumerate(dc.make_steps(c, 2)):
        net, _ = build(Unet, c, P)
        loss, pred, noisy = batch_loss(net, c, act[idx], t, eps, obs[idx])
        loss.backward()
        g32 = {k: p.grad.numpy().copy() for k, p in net.named_parameters()}
        net64, _ = build(OurUnet, c, P, torch.float64)
        loss64, pred64, _ = batch_loss(net64, c, act[idx], t, eps, obs[idx], torch.float64)
        loss64.backward()
        g64 = {k: p.grad.numpy().copy() for k, p in net64.named_parameters()}
        assert all(not np.delete(g, g.shape[2] // 2, axis=2).any() for g in g32.values() if g.ndim == 3 and g.shape[2] > 1)
        dist, noise = grad_distance(g32, g64)
        assert noise == 0.0                                            # every tensor has a gradient
        ol, op, og, _ = orc.loss_and_grads(P, c, act[idx], t, eps, obs[idx])
        od, _ = grad_distance(og, g64)
        print(f"(d) batch {b} ({len(idx)} rows): loss {loss.item():.6f}; fp32 vs float64 autograd {dist:.3e}; oracle: pred "
              f"{np.abs(op - pred.detach().numpy()[:, 0]).max():.2e} grads {od:.3e}; pred rows differ by {np.ptp(pred.detach().numpy()[:, 0], axis=0).max():.2f}")
        assert od <= 4 * dist
        out.update({f"b{b}/pred": pred.detach().numpy()[:, 0], f"b{b}/loss": np.float64(loss.item()), f"b{b}/loss64": np.float64(loss64.item()),
                    f"b{b}/x_t": noisy.numpy()[:, 0], f"b{b}/grad_f32_vs_f64": np.float64(dist)})
        out.update({f"b{b}/grad64/{k}": centre(v).astype(np.float32) for k, v in g64.items()})      # (rounded: 6e-8, far below the bar)
    sobs, snoise, sz = dc.make_sample_inputs(dict(c, rows=4))
    net, _ = build(Unet, c, P)
    out["actions"] = sample(net, c, sobs, snoise, sz)
    steps = dc.make_steps(c, c["steps"])
    losses, fin, ema = run_training(Unet, c, P, steps, c["steps"])
    twin = {k: np.nextafter(v, np.float32(np.inf)).astype(np.float32) for k, v in P.items()}
    tl, tfin, tema = run_training(Unet, c, twin, steps, c["steps"])
    olosses, ofin, oema = orc.train(P, c, dc.make_data(c), steps, c["steps"])
    print(f"(d) {c['steps']} steps: losses {losses[0]:.5f} .. {losses[-1]:.5f}; twin max |dloss| {np.abs(tl - losses).max():.2e}; oracle {np.abs(olosses - losses).max():.2e}")
    tr = {"losses": losses, "losses_twin": tl}
    for k in fin:
        tr[f"final/{k}"], tr[f"ema/{k}"], tr[f"final_twin/{k}"], tr[f"ema_twin/{k}"] = centre(fin[k]), centre(ema[k]), centre(tfin[k]), centre(tema[k])
    np.savez_compressed(os.path.join(HERE, "diffusion_d.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "diffusion_d_traj.npz"), **tr)
    # ---- (e): n_groups = 4 in the blocks, GroupNorm(8) in final_conv, from the reference's own module -------------------------------
    c = dc.CASES["e"]
    net, P = build(Unet, c)
    assert net.final_conv[0].block[1].num_groups == 8 and net.mid_modules[0].blocks[0].block[1].num_groups == 4
    obs, act = dc.make_data(c)
    idx, t, eps = dc.make_steps(c, 1)[0]
    loss, pred, noisy = batch_loss(net, c, act[idx], t, eps, obs[idx])
    loss.backward()
    g32 = {k: p.grad.numpy().copy() for k, p in net.named_parameters()}
    net64, _ = build(OurUnet, c, P, torch.float64)
    loss64, _, _ = batch_loss(net64, c, act[idx], t, eps, obs[idx], torch.float64)
    loss64.backward()
    g64 = {k: p.grad.numpy().copy() for k, p in net64.named_parameters()}
    dist, noise = grad_distance(g32, g64)
    ol, op, og, _ = orc.loss_and_grads(P, c, act[idx], t, eps, obs[idx])
    od, _ = grad_distance(og, g64)
    print(f"(e) parameters {sum(p.numel() for p in net.parameters())}; loss {loss.item():.6f}; fp32 vs float64 autograd {dist:.3e}; oracle grads {od:.3e}")
    assert noise == 0.0 and od <= 4 * dist
    out = {"pred": pred.detach().numpy()[:, 0], "loss": np.float64(loss.item()), "x_t": noisy.numpy()[:, 0], "grad_f32_vs_f64": np.float64(dist)}
    out.update({f"grad64/{k}": centre(v).astype(np.float32) for k, v in g64.items()})
    np.savez_compressed(os.path.join(HERE, "diffusion_e.npz"), **out)
    for f in ("a", "b", "c", "d", "d_traj", "e"):
        print(f"diffusion_{f}.npz", os.path.getsize(os.path.join(HERE, f"diffusion_{f}.npz")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])

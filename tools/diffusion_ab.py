#!/usr/bin/env python3
"""tools/diffusion_ab.py: are two builds of DiffusionBC (csrc/diffusion.hip) bit for bit the same on the GPU?

    ORL_ENGINE_LIB=<parent's library> python tools/diffusion_ab.py dump a.npz
    python tools/diffusion_ab.py dump b.npz                                 (fresh processes: one library per process)
    python tools/diffusion_ab.py cmp a.npz b.npz

``dump`` runs ONE fixed scenario at the shapes of tests/golden/diffusion_cases.py, cases (a) (down_dims [8, 16, 32]: a residual conv,
skip concatenations, groups of 1, 2 and 4 channels, act_dim 3) and (e) (n_groups 4 under final_conv's GroupNorm(8)), batch 6 over
8 rows.  Per case: two teacher-forced steps, two steps with device-drawn t / eps (one of 4 rows), a learn_epoch over the 8 rows (the
second minibatch is 2 rows) from a host order and from a device order, and sample on 5 rows from host arrays with given z and a
noise_idx, from host arrays with device-drawn z, from device tensors, then on 9 rows (the staging grows).  After every call it stores
params, EMA, both Adam blocks, debug_grads, every debug_read tap, what the call returned and step_count.  ``cmp`` is dyn_ab.py's:
32-bit patterns, non-zero exit on any difference.  Needs a GPU for ``dump``."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "offlinerl-kit_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dyn_ab import bits, cmp  # noqa: E402,F401

TAPS = ["pred", "x_t", "eps", "t", "gf", "film", "loss", "z", "x"]


def run_case(tag, c, out):
    import torch
    from offlinerlkit import _engine
    from offlinerlkit.policy.diffusion import ddpm_schedule, lr_table
    import diffusion_cases as dc
    rng = np.random.default_rng(c["seed"])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    cfg = _engine.default_diffusion_config(obs_dim=c["obs_dim"], act_dim=c["act_dim"], step_embed_dim=c["dsed"], down_dims=c["down_dims"],
                                           kernel_size=c["kernel_size"], n_groups=c["n_groups"], num_diffusion_iters=c["N"],
                                           batch_size=c["B"], seed=7)
    eng = _engine.Diffusion(cfg)
    _, acp, coef = ddpm_schedule(c["N"])
    eng.set_schedule(acp, coef)
    eng.set_lr(lr_table(20))
    flat = np.zeros(eng.floats, np.float32)
    for name, off, shape in eng.tensors():
        u = rng.uniform(-1.0, 1.0, size=shape)
        norm = ".block.1." in name
        v = ((1.0 if name.endswith("weight") else 0.0) + 0.3 * u) if norm else u / np.sqrt(shape[-1] if len(shape) == 2 else 8.0)
        flat[off:off + v.size] = f32(v).ravel()
    eng.set(eng.PARAMS, flat)
    eng.set(eng.EMA, flat)
    obs, act = dc.make_data(c)
    buf = _engine.DeviceBuffer(c["obs_dim"], c["act_dim"])
    zero = np.zeros(len(obs), np.float32)
    buf.load(obs, act, obs, zero, zero)
    eng.attach_buffer(buf)
    call_no = [0]

    def after(name, *returned):
        key = "%s/%02d_%s" % (tag, call_no[0], name)
        call_no[0] += 1
        for i, a in enumerate(returned):
            out["%s/ret%d" % (key, i)] = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        for which, nm in ((eng.PARAMS, "params"), (eng.EMA, "ema"), (eng.EXP_AVG, "exp_avg"), (eng.EXP_AVG_SQ, "exp_avg_sq")):
            out["%s/%s" % (key, nm)] = eng.get(which)
        out[key + "/grads"] = eng.debug_grads()
        out[key + "/step_count"] = np.asarray([eng.step_count], np.int64)
        for tap in TAPS:
            try:
                out["%s/tap_%s" % (key, tap)] = eng.debug_read(tap)
            except RuntimeError:                       # nothing recorded for it yet
                out["%s/tap_%s" % (key, tap)] = np.zeros(0, np.float32)

    after("init")
    for i, (idx, t, eps) in enumerate(dc.make_steps(c, 2)):
        after("step_forced%d" % i, eng.step(idx, t, eps))
    after("step_drawn0", eng.step(rng.permutation(c["n"])[:c["B"]]))
    after("step_drawn1", eng.step(rng.permutation(c["n"])[:4]))
    after("epoch_host", eng.learn_epoch(rng.permutation(c["n"])))
    dev = torch.device("cuda", 0)
    after("epoch_device", eng.learn_epoch(torch.as_tensor(rng.permutation(c["n"]).astype(np.int64), device=dev).contiguous()))
    ad, N = c["act_dim"], c["N"]
    normal = lambda *shape: f32(rng.standard_normal(shape))
    s_obs, noise, nidx = normal(5, c["obs_dim"]), normal(3, ad), rng.integers(0, 3, size=5).astype(np.int64)
    after("sample_host_z", eng.sample(s_obs, noise, noise_idx=nidx, z=normal(N, 5, ad)))
    after("sample_host_drawn", eng.sample(s_obs, normal(5, ad)))
    tdev = lambda a: torch.as_tensor(a, device=dev).contiguous()
    after("sample_device", eng.sample(tdev(s_obs), tdev(noise), noise_idx=tdev(nidx)))
    after("sample_grown", eng.sample(normal(9, c["obs_dim"]), normal(9, ad)))
    eng.close()
    buf.close()


def dump(path):
    import diffusion_cases as dc
    out = {}
    for tag in ("a", "e"):
        run_case(tag, dc.CASES[tag], out)
    np.savez(path, **out)
    print("diffusion_ab dump: %d arrays, %d values -> %s" % (len(out), sum(a.size for a in out.values()), path))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "cmp":
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)

#!/usr/bin/env python3
"""tools/dyn_ab.py: are two builds of the dynamics ensemble (csrc/dynamics.hip) bit for bit the same on the GPU?

    ORL_ENGINE_LIB=<parent's library> python tools/dyn_ab.py dump a.npz
    python tools/dyn_ab.py dump b.npz                                       (fresh processes: one library per process)
    python tools/dyn_ab.py cmp a.npz b.npz

``dump`` runs ONE fixed scenario through every orl_dyn* / orl_dynsample* / orl_dynadv* path and stores every output and, after each
stage, every run's parameters, ``debug_grads`` and both optimizers' m, v and step.  The shapes are the smallest that reach every guarded
path: obs 5 / act 2 (D = 6: the four-dim thread groups have a two-element tail; input width 7 is no multiple of 4), hidden [10, 7],
3 members with the elites [2, 0], 2 runs with their own weights and scalers, batch 8 over 19 training rows (a last minibatch of 3 rows
at a row stride of 8).  ``cmp`` compares every array as its 32-bit patterns (NaNs and signed zeros count), lists each differing key with
its first differing index and exits non-zero on any difference.  Needs a GPU for ``dump``."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "offlinerl-kit_amd"))

OD, AD, HID, K, ELITES, R, B, TRAIN = 5, 2, [10, 7], 3, [2, 0], 2, 8, 19
D = OD + 1


def dump(path):
    import torch
    from offlinerlkit import _engine
    rng = np.random.default_rng(20)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    normal = lambda *shape: f32(rng.normal(size=shape))
    cfg = _engine.default_dyn_config(obs_dim=OD, act_dim=AD, hidden=HID, num_ensemble=K, num_elites=len(ELITES), batch_size=B, n_runs=R,
                                     weight_decay=[2.5e-5, 5e-5, 7.5e-5], lr=1e-3, seed=11)
    eng = _engine.Dynamics(cfg)
    out, stage_no = {}, [0]

    def put(name, *arrays):
        for i, a in enumerate(arrays):
            out["%s/%d" % (name, i)] = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)

    def stage(name):
        """every run's parameters, last gradients and both optimizers' state"""
        tag = "state%02d_%s" % (stage_no[0], name)
        stage_no[0] += 1
        for r in range(R):
            states = [("adam", eng.adam_state(r))] + ([("adv_adam", eng.adv_adam_state(r))] if hasattr(eng, "adv_rows") else [])
            for k, v in eng.get_params(r).items():
                out["%s/r%d/param/%s" % (tag, r, k)] = v
            for k, v in eng.debug_grads(r).items():
                out["%s/r%d/grad/%s" % (tag, r, k)] = v
            for opt, (m, v, t) in states:
                out["%s/r%d/%s/step" % (tag, r, opt)] = np.asarray([t], np.int64)
                for k in m:
                    out["%s/r%d/%s/m/%s" % (tag, r, opt, k)] = m[k]
                    out["%s/r%d/%s/v/%s" % (tag, r, opt, k)] = v[k]

    for r in range(R):
        p = {}
        for name, _, shape in eng.tensors:
            if name == "max_logvar":
                p[name] = f32(0.5 + 0.1 * rng.normal(size=shape))
            elif name == "min_logvar":
                p[name] = f32(-10.0 + 0.1 * rng.normal(size=shape))
            elif "saved" in name:
                p[name] = np.zeros(shape, np.float32)
            else:
                p[name] = f32(rng.normal(size=shape) / np.sqrt(shape[1] if name.endswith("weight") else 4.0))
        eng.set_params(r, p)
        eng.set_elites(r, ELITES)
        eng.set_scaler(r, 0.3 * normal(OD + AD), f32(rng.uniform(0.5, 2.0, size=OD + AD)))
    rows = TRAIN + 6
    eng.load_data(normal(rows, OD + AD), 0.5 * normal(rows, D))
    stage("init")

    # learn: two epochs of 3 minibatches (8, 8, 3 rows), the second with run 1 frozen; validate on 5 rows
    put("learn0", eng.learn_epoch(rng.integers(0, rows, size=(R, K, TRAIN))))
    stage("learn0")
    put("learn1", eng.learn_epoch(rng.integers(0, rows, size=(R, K, TRAIN)), active=[1, 0]))
    stage("learn1")
    put("validate", eng.validate(rng.integers(0, rows, size=(R, 5))))

    # step: every penalty mode with host noise + teacher-forced members, then with the device Philox stream, then on device tensors
    n = 11
    obs, act = normal(R, n, OD), f32(rng.uniform(-1, 1, size=(R, n, AD)))
    modes = list(_engine.DYN_PENALTY)
    for m in modes:
        put("step_host_" + m, *eng.step(obs, act, noise=normal(R, K, n, D), model_idx=rng.integers(0, K, size=(R, n)), mode=m, coef=2.5))
    for m in modes:
        put("step_philox_" + m, *eng.step(obs, act, mode=m, coef=0.7))
    dev = torch.device("cuda", 0)
    tdev = lambda a: torch.as_tensor(a, device=dev).contiguous()
    put("step_device", *eng.step_device(tdev(obs), tdev(act), mode=modes[0], coef=1.5))

    # sample_next: 2 samples of every elite, host noise / device Philox, host / device arrays
    nz = normal(R, 2, len(ELITES), n, D)
    put("sample_host_noise", eng.sample_next(obs, act, 2, noise=nz))
    put("sample_host_philox", eng.sample_next(obs, act, 2))
    put("sample_device_noise", eng.sample_next_device(tdev(obs), tdev(act), 2, noise=tdev(nz)))
    put("sample_device_philox", eng.sample_next_device(tdev(obs), tdev(act), 2))

    # adversarial update: 5 rollout + 7 dataset rows
    Ba, Bs = 5, 7
    configure = lambda: eng.adv_configure(3e-4, adv_weight=3e-4, rollout_rows=Ba, sl_rows=Bs)
    batch = lambda: (normal(R, Ba, OD), f32(rng.uniform(-1, 1, size=(R, Ba, AD))), normal(R, Bs, OD),
                     f32(rng.uniform(-1, 1, size=(R, Bs, AD))), normal(R, Bs, OD), normal(R, Bs))
    configure()
    put("adv0_forward", *eng.adv_forward(*batch(), noise=normal(R, K, Ba, D), model_idx=rng.integers(0, K, size=(R, Ba))))
    put("adv0_step_between", *eng.step(obs, act, mode=modes[0], coef=1.0))      # the three call counters do not disturb each other
    put("adv0_update", eng.adv_update(normal(R, Ba)))
    stage("adv0")
    put("adv1_forward", *eng.adv_forward(*batch()))
    configure()                                                                 # unchanged row counts: the forward stays pending
    put("adv1_update", eng.adv_update(normal(R, Ba), active=[0, 1]))
    stage("adv1")
    put("adv2_forward", *eng.adv_forward_device(*[tdev(a) for a in batch()]))
    put("adv2_update", eng.adv_update_device(tdev(normal(R, Ba))))
    stage("adv2")
    eng.close()
    np.savez(path, **out)
    print("dyn_ab dump: %d arrays, %d values -> %s" % (len(out), sum(a.size for a in out.values()), path))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).ravel() if a.dtype.kind == "f" else a.ravel()


def cmp(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print("%s: only in one file" % k)
    total = 0
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        total += x.size
        if x.shape != y.shape or x.dtype != y.dtype:
            print("%s: %s %s against %s %s" % (k, x.dtype, x.shape, y.dtype, y.shape))
            bad.append(k)
            continue
        ne = np.flatnonzero(bits(x) != bits(y))
        if ne.size:
            i = int(ne[0])
            print("%s: %d of %d differ, first at %d: %r against %r" % (k, ne.size, x.size, i, x.ravel()[i], y.ravel()[i]))
            bad.append(k)
    print("dyn_ab cmp: %d arrays, %d values compared as bit patterns, %d arrays differ" % (len(a.files), total, len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "cmp":
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)

#!/usr/bin/env python3
"""Golden fixtures of the REAL reference termination functions and MBPolicyTrainer (build container only).

``mb_termination.npz``: every ``termination_fn_*`` on the rows of ``mb_trainer_fakes.term_inputs`` and the function
``get_termination_fn`` picks for each task name.  ``mb_trainer_trace.npz``: the reference MBPolicyTrainer + Logger + ReplayBuffer driven
by the duck-typed fakes of ``mb_trainer_fakes`` (CSV, the sums of every rollout-init / real / model draw, the rollout log lines, the
model buffer after each rollout, checkpoints and the dynamics.save call).  ``gym`` / ``gymnasium`` / tensorboard are stubbed as in
make_trainer_golden.py; only the trainer, logger, buffer and termination code of the reference runs.
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import mb_trainer_fakes as mf  # noqa: E402


def _stubs():
    def stub(name, **attrs):
        m = types.ModuleType(name); m.__dict__.update(attrs); sys.modules[name] = m; return m

    class _X:
        pass

    stub("gym", spaces=stub("gym.spaces", Space=_X), Env=_X)
    stub("gymnasium", Env=_X)

    class SummaryWriter:
        def __init__(self, *a, **k): pass
        def add_scalar(self, *a, **k): pass
        def add_hparams(self, *a, **k): pass
        def flush(self): pass
        def close(self): pass
    import torch.utils  # noqa: F401
    stub("torch.utils.tensorboard", SummaryWriter=SummaryWriter)
    pkg = types.ModuleType("offlinerlkit.policy")
    pkg.__path__ = ["/root/reference/offlinerlkit/policy"]
    sys.modules["offlinerlkit.policy"] = pkg
    pkg.BasePolicy = importlib.import_module("offlinerlkit.policy.base_policy").BasePolicy
    tr = types.ModuleType("offlinerlkit.policy_trainer"); tr.__path__ = ["/root/reference/offlinerlkit/policy_trainer"]
    sys.modules["offlinerlkit.policy_trainer"] = tr


def termination(tf_mod):
    obs, act, nxt = mf.term_inputs()
    out = {"obs": obs, "act": act, "next_obs": nxt}
    for name in mf.TERM_FNS:
        out["fn_" + name] = np.asarray(getattr(tf_mod, "termination_fn_" + name)(obs, act, nxt))
    out["door_is_none"] = np.array([tf_mod.termination_fn_door(obs, act, nxt) is None])
    out["task_fn"] = np.array([tf_mod.get_termination_fn(t).__name__ for t in mf.TASKS])
    np.savez_compressed(os.path.join(HERE, "mb_termination.npz"), **out)


def trainer(logger_mod, ReplayBuffer, MBPolicyTrainer):
    out = {}
    snaps = []

    class FakeBuffer(ReplayBuffer):
        def add_batch(self, *a, **k):
            super().add_batch(*a, **k)
            snaps.append(np.concatenate([self.observations, self.next_observations, self.actions, self.rewards, self.terminals], 1).copy())
            snaps.append(np.array([[self._ptr, self._size] + [0] * (2 * mf.OBS + mf.ACT)], np.float64))

    with tempfile.TemporaryDirectory() as d:
        logger = logger_mod.Logger(d, {"consoleout_backup": "stdout", "policy_training_progress": "csv",
                                       "dynamics_training_progress": "csv"})
        lines = []
        logger.log = lambda s, *a, **k: lines.append(s)
        real = ReplayBuffer(mf.N_DATA, (mf.OBS,), np.float32, mf.ACT, np.float32, device="cpu")
        real.load_dataset(mf.dataset())
        fake = FakeBuffer(mf.FAKE_CAP, (mf.OBS,), np.float32, mf.ACT, np.float32, device="cpu")
        pol, sched = mf.FakePolicy(), mf.FakeScheduler()
        np.random.seed(mf.SEED)
        res = MBPolicyTrainer(pol, mf.FakeEnv(), real, fake, logger, mf.ROLLOUT, epoch=mf.EPOCHS, step_per_epoch=mf.STEPS,
                              batch_size=mf.BATCH, real_ratio=mf.REAL_RATIO, eval_episodes=mf.EVAL_EPS, lr_scheduler=sched).train()
        with open(os.path.join(d, "record", "policy_training_progress.csv")) as f:
            csv_text = f.read()
        out["ckpt_exists"] = np.array([os.path.exists(os.path.join(d, "checkpoint", "policy.pth")),
                                       os.path.exists(os.path.join(d, "model", "policy.pth")),
                                       os.path.exists(os.path.join(d, "model", "dynamics.pth"))])
    out["last_10_performance"] = np.array([res["last_10_performance"]])
    out["sched_steps"] = np.array([sched.n])
    out["init_sums"], out["real_sums"], out["fake_sums"] = (np.array(x) for x in (pol.init_sums, pol.real_sums, pol.fake_sums))
    out["rollout_lines"] = np.array([s for s in lines if s.startswith("num rollout")])
    out["dyn_saved"] = np.array(pol.dynamics.saved)
    out["fake_snapshots"] = np.stack(snaps[0::2])
    out["fake_ptr_size"] = np.stack(snaps[1::2])[:, 0, :2]
    lines_csv = csv_text.strip().split("\n")
    out["csv_header"] = np.array(lines_csv[0].split(","))
    out["csv_rows"] = np.array([[float(x) if x else np.nan for x in ln.split(",")] for ln in lines_csv[1:]])
    np.savez_compressed(os.path.join(HERE, "mb_trainer_trace.npz"), **out)
    print("header:", lines_csv[0]); print("rows:", out["csv_rows"].shape, "rollouts:", len(out["init_sums"]))


def main():
    sys.path.insert(0, "/root/reference")
    _stubs()
    termination(importlib.import_module("offlinerlkit.utils.termination_fns"))
    logger_mod = importlib.import_module("offlinerlkit.utils.logger")
    MBPolicyTrainer = importlib.import_module("offlinerlkit.policy_trainer.mb_policy_trainer").MBPolicyTrainer
    from offlinerlkit.buffer import ReplayBuffer
    trainer(logger_mod, ReplayBuffer, MBPolicyTrainer)


if __name__ == "__main__":
    main()

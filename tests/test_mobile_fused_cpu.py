"""CPU: MOBILEDevicePolicy's surface -- the fused entry points, the reference's state_dict keys, what MBPolicyTrainer(fused=True)
accepts and refuses -- and the C ABI of the device loop behind it (orl_mobile_learn_n).  No compute calls (there is no GPU here)."""
import os
import re

import pytest
import torch

from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _policy(cls_name, dynamics=None):
    from offlinerlkit import policy as pk
    from offlinerlkit.modules import ActorProb, Critic, TanhDiagGaussian
    from offlinerlkit.nets import MLP
    od, ad, hid = 5, 2, [32, 32]
    actor = ActorProb(MLP(od, hid), TanhDiagGaussian(hid[-1], ad, unbounded=True, conditioned_sigma=True), "cpu")
    critics = torch.nn.ModuleList([Critic(MLP(od + ad, hid), "cpu") for _ in range(2)])
    return getattr(pk, cls_name)(dynamics if dynamics is not None else object(), actor, critics, torch.optim.Adam(actor.parameters(), lr=1e-4),
                                 torch.optim.Adam(critics.parameters(), lr=3e-4), penalty_coef=1.5, num_samples=10, deterministic_backup=True)


def test_device_policy_has_the_fused_entry_points_and_the_references_state_dict():
    from offlinerlkit.policy import MOBILEDevicePolicy, MOBILEPolicy
    assert issubclass(MOBILEDevicePolicy, MOBILEPolicy)
    pol = _policy("MOBILEDevicePolicy")
    assert callable(pol.learn_n) and callable(pol.rollout_device)
    for name in ("learn", "compute_lcb", "rollout", "state_dict"):
        assert getattr(MOBILEDevicePolicy, name) is getattr(MOBILEPolicy, name), name
    g = load_golden("mobile_tiny")
    assert list(pol.state_dict().keys()) == [str(k) for k in g["state_keys"]]
    assert {k.split(".")[0] + "." + k.split(".")[1] for k in pol.state_dict() if not k.startswith("actor.")} == \
        {"critics.0", "critics.1", "critics_old.0", "critics_old.1"}
    assert any(k.startswith("actor.") for k in pol.state_dict())
    # the plain policy keeps refusing both
    plain = _policy("MOBILEPolicy")
    assert not hasattr(plain, "learn_n") and not hasattr(plain, "rollout_device")


class _Ring:
    def reserve_device(self):
        return None


def test_fused_trainer_takes_the_device_policy_and_still_refuses_the_plain_one():
    import mb_trainer_fakes as fk
    from offlinerlkit.policy_trainer import MBPolicyTrainer
    from offlinerlkit.utils import termination_fns as tf

    class Dyn:
        term_kind = tf.term_kind(tf.termination_fn_halfcheetah)
    kw = dict(epoch=1, step_per_epoch=fk.STEPS, batch_size=fk.BATCH, real_ratio=fk.REAL_RATIO, eval_episodes=1)
    MBPolicyTrainer(_policy("MOBILEDevicePolicy", Dyn()), fk.FakeEnv(), object(), _Ring(), None, fk.ROLLOUT, fused=True, **kw)
    MBPolicyTrainer(_policy("MOBILEDevicePolicy", Dyn()), fk.FakeEnv(), object(), _Ring(), None, fk.ROLLOUT, fused=False, **kw)
    with pytest.raises(ValueError, match="rollout_device"):
        MBPolicyTrainer(_policy("MOBILEPolicy", Dyn()), fk.FakeEnv(), object(), _Ring(), None, fk.ROLLOUT, fused=True, **kw)


def test_several_runs_and_per_run_rings_are_refused():
    pol = _policy("MOBILEDevicePolicy")
    with pytest.raises(NotImplementedError, match="n_runs"):
        pol.set_engine_options(n_runs=2)
    pol.set_engine_options(n_runs=1, precision=0)
    for call in (lambda fake: pol.learn_n(3, object(), fake, 16, 0.25), lambda fake: pol.rollout_device(object(), fake, 8, 2)):
        with pytest.raises(NotImplementedError, match="one model ring"):
            call([_Ring()])
        with pytest.raises(NotImplementedError, match="one model ring"):
            call((_Ring(), _Ring()))

    class TwoRuns:
        _n_runs = 2
    pol2 = _policy("MOBILEDevicePolicy", TwoRuns())
    with pytest.raises(NotImplementedError, match="n_runs == 1"):
        pol2.learn_n(3, object(), _Ring(), 16, 0.25)
    with pytest.raises(NotImplementedError, match="n_runs == 1"):
        pol2.rollout_device(object(), _Ring(), 8, 2)
    with pytest.raises(NotImplementedError, match="real and a model-rollout buffer"):
        pol.learn_n(3, object())


def test_header_declares_and_library_exports_the_device_loop():
    import importlib.util
    spec = importlib.util.spec_from_file_location("orl_build", os.path.join(ROOT, "offlinerl-kit_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from offlinerlkit import _engine
    lib = _engine.load_library()
    header = open(os.path.join(ROOT, "include", "orl_engine.h")).read()
    declared = set(re.findall(r"\b(orl_[a-z0-9_]+)\s*\(", header))
    for sym in ("orl_mobile_learn_n", "orl_dynsample_calls"):
        assert sym in declared and sym in _engine.ABI_SYMBOLS and hasattr(lib, sym), sym
    assert re.search(r"int\s+orl_mobile_learn_n\(orl_engine\*\s*e,\s*orl_dynamics\*\s*d,\s*int\s+n_steps,\s*float\*\s*metrics_mean[^,]*,\s*"
                     r"float\*\s*elapsed_ms\)", header)
    assert hasattr(_engine.Engine, "mobile_learn_n") and hasattr(_engine.Dynamics, "sample_calls")

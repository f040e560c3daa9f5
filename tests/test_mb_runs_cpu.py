"""CPU: what the per-run model rings (a sequence of ``n_runs`` buffers as ``fake_buffer``) refuse at construction or at the call, with
the stub objects of test_mb_fused_cpu.py, and the ABI declarations of the two entry points."""
import os

import numpy as np
import pytest

import mb_trainer_fakes as fk


class _RunsPolicy(fk.FakePolicy):
    n_runs = 3

    def rollout_device(self, *a, **k):
        raise AssertionError("not reached")

    def learn_n(self, *a, **k):
        raise AssertionError("not reached")


class _KindDynamics(fk.FakeDynamics):
    def __init__(self, n_runs=1):
        super().__init__()
        self._n_runs = n_runs

    @property
    def term_kind(self):
        from offlinerlkit.utils import termination_fns as tf
        return tf.TERM_HALFCHEETAH

    def step_device_runs(self, o, a):
        raise AssertionError("not reached")


def _buf(cap=50, od=fk.OBS, ad=fk.ACT, device="cpu"):
    from offlinerlkit.buffer import ReplayBuffer
    return ReplayBuffer(cap, (od,), np.float32, ad, np.float32, device=device)


def _trainer(policy, fake, **kw):
    from offlinerlkit.policy_trainer import MBPolicyTrainer
    return MBPolicyTrainer(policy, fk.FakeEnv(), object(), fake, None, fk.ROLLOUT, epoch=1, step_per_epoch=fk.STEPS, batch_size=fk.BATCH,
                           real_ratio=fk.REAL_RATIO, eval_episodes=1, **kw)


def _policy(dyn_runs=3):
    pol = _RunsPolicy()
    pol.dynamics = _KindDynamics(dyn_runs)
    return pol


def test_trainer_refuses_a_sequence_of_the_wrong_length():
    for n in (1, 2, 4):
        with pytest.raises(ValueError, match="n_runs = 3"):
            _trainer(_policy(), [_buf() for _ in range(n)], fused=True)
    with pytest.raises(ValueError, match="n_runs = 3"):
        _trainer(_policy(), tuple(_buf() for _ in range(2)), fused=True)
    b = _buf()
    with pytest.raises(ValueError, match="twice"):
        _trainer(_policy(), [b, _buf(), b], fused=True)


def test_trainer_refuses_per_run_rings_on_the_host_loop():
    with pytest.raises(ValueError, match="fused=True.*single-buffer"):
        _trainer(_policy(), [_buf() for _ in range(3)], fused=False)
    with pytest.raises(ValueError, match="fused=True.*single-buffer"):
        _trainer(_policy(), [_buf() for _ in range(3)])                  # (fused defaults to False)
    _trainer(_policy(), _buf())                                          # one buffer: the reference's loop, as before


@pytest.mark.parametrize("other", [dict(od=fk.OBS + 1), dict(ad=fk.ACT + 1), dict(cap=51), dict(device="cuda:0")])
def test_trainer_refuses_rings_that_differ(other):
    with pytest.raises(ValueError, match="run 1's buffer.*differs"):
        _trainer(_policy(), [_buf(), _buf(**other), _buf()], fused=True)


def test_trainer_refuses_a_dynamics_of_another_run_count():
    for runs in (2, 4):
        with pytest.raises(ValueError, match=f"carries {runs}"):
            _trainer(_policy(runs), [_buf() for _ in range(3)], fused=True)


def test_policy_entry_points_refuse_the_same_sequences():
    """learn_n and rollout_device check the sequence before they touch the device"""
    from offlinerlkit.policy import COMBOPolicy, MOPOPolicy
    from offlinerlkit.policy import model_based as mb
    for cls in (MOPOPolicy, COMBOPolicy):
        pol = cls.__new__(cls)
        pol._n_runs = 3
        pol._rows = None
        pol._eng = None
        pol._uniform_rollout = False
        pol.dynamics = _KindDynamics(3)
        for bad, what in (([_buf(), _buf()], "n_runs = 3"), ([_buf(), _buf(cap=7), _buf()], "differs")):
            with pytest.raises(ValueError, match=what):
                pol.rollout_device(object(), bad, 4, 1)
            with pytest.raises(ValueError, match=what):
                mb._learn_n_mb(pol, 1, object(), bad, 16, 0.5)
    assert mb.per_run_rings(pol, _buf()) is None and mb.per_run_rings(pol, object()) is None
    rings = [_buf() for _ in range(3)]
    assert mb.per_run_rings(pol, rings) == rings
    # a dynamics of another run count is refused before any device work
    pol.dynamics = _KindDynamics(2)
    with pytest.raises(ValueError, match="carries 2 runs"):
        mb._rollout_device_runs(pol, object(), rings, 4, 1, np.zeros((12, fk.OBS), np.float32), False)


def test_the_two_entry_points_are_declared_and_listed():
    from offlinerlkit import _engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "orl_engine.h")).read()
    for name in ("orl_buffer_append_rollout_runs", "orl_engine_attach_model_buffers"):
        assert name in _engine.ABI_SYMBOLS and f"int {name}(" in header
    assert hasattr(_engine.Engine, "attach_model_buffers") and hasattr(_engine.DeviceBuffer, "append_rollout_runs")

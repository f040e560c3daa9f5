"""CPU: the chunk arithmetic of MBPolicyTrainer(fused=True) against a brute-force walk of the reference loop
(mb_policy_trainer.py:66-102), and the configurations the fused loop refuses at construction."""

import pytest

import mb_trainer_fakes as fk


@pytest.mark.parametrize("rollout_freq", [1, 3, 7, 1000])
@pytest.mark.parametrize("step_per_epoch", [7, 250, 1000])
def test_fused_schedule_is_the_reference_loop_cut_at_the_rollouts(rollout_freq, step_per_epoch):
    from offlinerlkit.policy_trainer import fused_mb_schedule
    t = 0
    for _ in range(3):
        # the reference loop, event by event: "R" in front of a timestep that rolls out, "s" per training step
        want, tt = [], t
        for _ in range(step_per_epoch):
            if tt % rollout_freq == 0:
                want.append(("R", tt))
            want.append(("s", tt))
            tt += 1
        got, tt = [], t
        chunks = fused_mb_schedule(t, step_per_epoch, rollout_freq)
        for rollout_first, n in chunks:
            assert n > 0                                            # no empty chunk
            if rollout_first:
                got.append(("R", tt))
            for _ in range(n):
                got.append(("s", tt))
                tt += 1
        assert got == want
        assert sum(n for _, n in chunks) == step_per_epoch
        assert [x for k, x in got if k == "R"] == [x for x in range(t, t + step_per_epoch) if x % rollout_freq == 0]
        t += step_per_epoch


class _DevicePolicy(fk.FakePolicy):
    def rollout_device(self, *a, **k):
        raise AssertionError("not reached")

    def learn_n(self, *a, **k):
        raise AssertionError("not reached")


class _KindDynamics(fk.FakeDynamics):
    def __init__(self, fn):
        super().__init__()
        self.terminal_fn = fn

    @property
    def term_kind(self):
        from offlinerlkit.utils import termination_fns
        return termination_fns.term_kind(self.terminal_fn)


def _trainer(policy, **kw):
    from offlinerlkit.policy_trainer import MBPolicyTrainer
    return MBPolicyTrainer(policy, fk.FakeEnv(), object(), object(), None, fk.ROLLOUT, epoch=1, step_per_epoch=fk.STEPS, batch_size=fk.BATCH,
                           real_ratio=fk.REAL_RATIO, eval_episodes=1, **kw)


def test_fused_refuses_dynamics_updates_missing_rollout_device_and_untagged_termination():
    from offlinerlkit.utils import termination_fns as tf
    pol = _DevicePolicy()
    pol.dynamics = _KindDynamics(tf.termination_fn_halfcheetah)
    with pytest.raises(ValueError, match="dynamics_update_freq"):
        _trainer(pol, fused=True, dynamics_update_freq=1)
    with pytest.raises(ValueError, match="rollout_device"):
        _trainer(fk.FakePolicy(), fused=True)
    # no kind: a dynamics that does not know the notion, a wrapper, door, any other callable
    with pytest.raises(ValueError, match="term_kind"):
        _trainer(_DevicePolicy(), fused=True)
    for fn in (tf.obs_unnormalization(tf.termination_fn_hopper, 0.0, 1.0), tf.termination_fn_door, lambda o, a, n: None):
        pol.dynamics = _KindDynamics(fn)
        with pytest.raises(ValueError, match="term_kind"):
            _trainer(pol, fused=True)
    # the default path takes none of these checks
    _trainer(fk.FakePolicy(), dynamics_update_freq=1)
    _trainer(fk.FakePolicy())


def test_model_based_policies_have_the_fused_entry_points():
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.policy import COMBOPolicy, MOPOPolicy
    from offlinerlkit.utils import termination_fns as tf
    import inspect
    for cls in (MOPOPolicy, COMBOPolicy):
        assert list(inspect.signature(cls.learn_n).parameters)[1:] == ["n_steps", "real_buffer", "fake_buffer", "batch_size", "real_ratio"]
        assert list(inspect.signature(cls.rollout_device).parameters)[1:] == ["real_buffer", "fake_buffer", "rollout_batch_size",
                                                                              "rollout_length", "init_obss"]
    dyn = EnsembleDynamics.__new__(EnsembleDynamics)
    dyn.terminal_fn = tf.termination_fn_walker2d
    assert dyn.term_kind == tf.TERM_WALKER2D
    dyn.terminal_fn = tf.obs_unnormalization(tf.termination_fn_walker2d, 0.0, 1.0)
    assert dyn.term_kind is None

"""GPU, end to end: MBPolicyTrainer with the real MOPOPolicy / COMBOPolicy, an EnsembleDynamics trained on the data and this package's
ReplayBuffer for the real and the model rows, on the point-mass task of tests/test_gpu_training.py.  Checks the wiring of the reference
loop (mb_policy_trainer.py:57-131) on the device objects: the reference's CSV keys, finite losses and returns, the rollout log lines,
the model buffer filling at the rollout timesteps, policy.pth / dynamics.pth, and the multi-run keys / checkpoints."""
import numpy as np
import pytest
import torch

from test_gpu_training import AD, DEV, HID, OD, PointMass, Space, make_dataset

pytestmark = pytest.mark.gpu
ROLLOUT = (100, 1000, 3)                  # rollout_freq, rollout_batch_size, rollout_length


def _dynamics(ds, logger):
    from offlinerlkit.dynamics import EnsembleDynamics
    from offlinerlkit.modules import EnsembleDynamicsModel
    from offlinerlkit.utils.scaler import StandardScaler
    from offlinerlkit.utils.termination_fns import get_termination_fn
    model = EnsembleDynamicsModel(OD, AD, [64, 64], num_ensemble=5, num_elites=3, weight_decays=[2.5e-5, 5e-5, 1e-4], device=DEV)
    dyn = EnsembleDynamics(model, torch.optim.Adam(model.parameters(), lr=1e-3), StandardScaler(), get_termination_fn("point2denv"),
                           penalty_coef=0.5, uncertainty_mode="aleatoric")
    dyn.train(ds, logger, max_epochs=15, max_epochs_since_update=5)
    return dyn


def _policy(algo, dyn):
    from offlinerlkit.modules import ActorProb, Critic, TanhDiagGaussian
    from offlinerlkit.nets import MLP
    from offlinerlkit.policy import COMBOPolicy, MOPOPolicy
    adam = lambda m, lr: torch.optim.Adam(m.parameters(), lr=lr)
    actor = ActorProb(MLP(OD, HID), TanhDiagGaussian(HID[-1], AD, unbounded=True, conditioned_sigma=True), DEV)
    c1, c2 = Critic(MLP(OD + AD, HID), DEV), Critic(MLP(OD + AD, HID), DEV)
    log_alpha = torch.zeros(1, requires_grad=True, device=DEV)
    alpha = (-float(AD), log_alpha, torch.optim.Adam([log_alpha], lr=1e-3))
    if algo == "mopo":         # run_example/run_mopo.py
        return MOPOPolicy(dyn, actor, c1, c2, adam(actor, 1e-3), adam(c1, 1e-3), adam(c2, 1e-3), tau=0.005, gamma=0.95, alpha=alpha)
    return COMBOPolicy(dyn, actor, c1, c2, adam(actor, 1e-3), adam(c1, 1e-3), adam(c2, 1e-3), Space(AD), tau=0.005, gamma=0.95,   # run_combo.py
                       alpha=alpha, cql_weight=1.0, temperature=1.0, max_q_backup=False, deterministic_backup=True, with_lagrange=False,
                       num_repeart_actions=4, uniform_rollout=False, rho_s="mix")


@pytest.mark.parametrize("algo,n_runs,real_ratio", [("mopo", 1, 0.05), ("combo", 1, 0.5), ("mopo", 2, 0.05)])
def test_mb_trainer_end_to_end(tmp_path, algo, n_runs, real_ratio):
    from offlinerlkit.buffer import ReplayBuffer
    from offlinerlkit.policy_trainer import MBPolicyTrainer
    from offlinerlkit.utils.logger import Logger
    torch.manual_seed(3)
    np.random.seed(3)
    ds = make_dataset(n_episodes=300)
    logger = Logger(str(tmp_path), {"consoleout_backup": "stdout", "policy_training_progress": "csv", "dynamics_training_progress": "csv"})
    real = ReplayBuffer(len(ds["rewards"]), (OD,), np.float32, AD, np.float32, device=DEV)
    real.load_dataset(ds)
    dyn = _dynamics(real.sample_all(), logger)
    pol = _policy(algo, dyn)
    if n_runs > 1:
        pol.set_engine_options(n_runs=n_runs, seed=11)
    fake = ReplayBuffer(ROLLOUT[1] * ROLLOUT[2] * 2, (OD,), np.float32, AD, np.float32, device=DEV)
    lines = []
    log = logger.log
    logger.log = lambda s, *a, **k: (lines.append(s), log(s, *a, **k))

    class Env(PointMass):
        def get_normalized_score(self, x):
            return x / 20.0

    epochs, steps = 2, 250
    res = MBPolicyTrainer(pol, Env(1000), real, fake, logger, ROLLOUT, epoch=epochs, step_per_epoch=steps, batch_size=256,
                          real_ratio=real_ratio, eval_episodes=5).train()
    rows = [ln.split(",") for ln in open(tmp_path / "record" / "policy_training_progress.csv").read().strip().split("\n")]
    head = rows[0]
    losses = ["loss/actor", "loss/critic1", "loss/critic2"] + (["loss/alpha", "alpha"] if algo == "mopo" else [])
    evals = ["eval/normalized_episode_reward", "eval/normalized_episode_reward_std", "eval/episode_length", "eval/episode_length_std"]
    want = set(losses + evals + ["rollout_info/num_transitions", "rollout_info/reward_mean", "timestep"])
    assert want <= set(head), want - set(head)
    assert "eval/episode_reward" not in head                                      # the reference's non-gymnasium branch
    if n_runs > 1:
        assert {f"run{r}/{k}" for r in range(n_runs) for k in evals} <= set(head)
        for r in range(n_runs):
            assert (tmp_path / "model" / f"policy_run{r}.pth").exists()
    col = lambda k: np.array([float(x[head.index(k)]) for x in rows[1:]])
    for k in losses + evals:
        assert np.isfinite(col(k)).all(), k
    assert list(col("timestep")) == [steps * (e + 1) for e in range(epochs)]
    # rollouts at timesteps 0, 100, ..., 400: 5 of them, every one rolls 1000 x 3 rows (point2denv never terminates)
    rl = [s for s in lines if s.startswith("num rollout transitions: ")]
    assert len(rl) == 5 and all(s.startswith("num rollout transitions: 3000,") for s in rl), rl
    assert np.allclose(col("rollout_info/num_transitions"), 3000.0)
    assert fake._size == fake._max_size == 6000 and np.isfinite(fake.rewards).all()
    for p in ("checkpoint/policy.pth", "model/policy.pth", "model/dynamics.pth"):
        assert (tmp_path / p).exists(), p
    assert np.isfinite(res["last_10_performance"])
    print(f"{algo} x{n_runs}: normalised eval return per epoch {col('eval/normalized_episode_reward').round(2).tolist()}")

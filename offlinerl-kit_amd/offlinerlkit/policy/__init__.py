"""offlinerlkit.policy — the four model-free policies of the hot path plus SAC and the model-based callers whose ``learn`` reuses
its kernels (MOPO, COMBO, MCQ: SURVEY §8(f)3), engine-backed, and RAMBO, whose adversarial update of the dynamics ensemble runs on the
dynamics engine (``orl_dynadv_*``), and MOBILE, whose penalty pass runs on the dynamics engine (``orl_dynsample_next``) and the policy
engine (``ORL_ALGO_MOBILE``), and RCSL's return-conditioned policies: the deterministic one (``ORL_ALGO_RCSL``: one MLP on [obs | rtg],
MSE on the dataset action) and the Gaussian one (``ORL_ALGO_RCSL_GAUSS``: the same MLP down to a latent, a DiagGaussian head with a
clamped state-conditioned sigma, Gaussian NLL); ``learn_epoch`` is one ordered pass over the dataset (``orl_learn_epoch``).  Their
``rollout`` rolls a behaviour policy through a dynamics model; the behaviour policy here is ``AutoregressivePolicy``
(``ORL_ALGO_AUTOREG``: p(a | s) as a product of per-dimension Gaussians from one LeakyReLU net, trained on the act_dim-fold expanded
batch and sampled by ``orl_autoreg_sample``).  ``rollout_device`` is that rollout with every array in HBM: ``select_action_device``,
``EnsembleDynamics.step_device`` and the trajectory store (``orl_traj_*``: per-row trajectory index, accumulated return and return-to-go,
float64 returns), whose thresholded export is the ``DeviceBuffer`` ``learn_epoch`` reads; ``rcsl.collect_rollouts_device`` loops the two.
``DiffusionBC`` is the pipeline's default behaviour policy: a DDPM over actions whose noise-prediction U-Net, at the sequence length 1
it is used at, trains and samples on ``orl_diffusion_*``; its frozen per-trajectory noise stays in HBM through ``rollout_device``."""
from .base_policy import BasePolicy, EnginePolicy
from .iql import IQLPolicy
from .sac_family import CQLPolicy, EDACPolicy
from .td3bc import TD3BCPolicy
from .model_based import SACPolicy, MOPOPolicy, COMBOPolicy
from .mcq import MCQPolicy
from .rambo import RAMBOPolicy, rambo_adv_schedule
from .mobile import MOBILEDevicePolicy, MOBILEPolicy
from .rcsl import RcslPolicy, RcslGaussianPolicy
from .autoregressive import AutoregressivePolicy
from .diffusion import DiffusionBC

__all__ = ["BasePolicy", "EnginePolicy", "CQLPolicy", "IQLPolicy", "TD3BCPolicy", "EDACPolicy", "SACPolicy", "MOPOPolicy", "COMBOPolicy", "MCQPolicy",
           "RAMBOPolicy", "MOBILEPolicy", "MOBILEDevicePolicy", "RcslPolicy", "RcslGaussianPolicy", "AutoregressivePolicy", "DiffusionBC"]

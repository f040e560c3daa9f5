"""MOBILE (reference: policy/model_based/mobile.py:14-196) on the HIP engines.

One ``learn`` is three calls, and the next-state samples never visit the host between them:
  1. ``EnsembleDynamics.sample_next_obss_device`` (``orl_dynsample_next``): the ensemble forward on the mixed batch and ``num_samples``
     draws of every elite's next observation, ``(S, E, B, obs_dim)`` on the device;
  2. ``orl_engine_set_next_samples``: the policy engine borrows that array;
  3. ``orl_step`` of an ``ORL_ALGO_MOBILE`` engine: the penalty pass (actor and the two target critics on the ``S * E * B`` samples,
     mean over samples -> unbiased std over elites per batch row, zero on the real rows), then SAC's update with the penalised,
     clamped target and one loss over both critics.
``compute_lcb`` is the penalty pass alone (``orl_engine_lcb_penalty``).

Exactly two critics (``--num-q-ensemble``'s default) and one run per policy.  ``MOBILEPolicy`` has no ``learn_n`` / ``rollout_device``:
``MBPolicyTrainer(fused=True)`` refuses it and ``fused=False`` trains it through the three calls above.

``MOBILEDevicePolicy`` is the same policy with the fused epoch: ``learn_n`` is ``orl_mobile_learn_n``, whole steps as one device loop on
the engine's stream.  Each step draws its batch from the dataset buffer and the model ring as ``orl_learn_n`` does, runs the ensemble
forward on the drawn rows and lets ``k_dyn_sample_rows`` write the ``S * E * B`` samples straight into the actor's and the target
critics' input rows of the penalty pass (no sample array, no assemble launch; the same bits as calls 1-2), then the launches of call 3.
One host synchronisation per ``learn_n``.  ``rollout_device`` is MOPO's device rollout.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from .. import _engine
from .base_policy import _backbone_dims, clone_target
from .model_based import _cat, _rollout, _rollout_device_any
from .sac_family import _TanhGaussPolicy


class MOBILEPolicy(_TanhGaussPolicy):
    """Model-Bellman Inconsistency Penalized Offline Reinforcement Learning; constructor = mobile.py:19-57."""

    ALGO = "mobile"

    def __init__(self, dynamics, actor: nn.Module, critics: nn.ModuleList, actor_optim, critics_optim, tau: float = 0.005,
                 gamma: float = 0.99, alpha: Union[float, Tuple] = 0.2, penalty_coef: float = 1.0, num_samples: int = 10,
                 deterministic_backup: bool = False) -> None:
        super().__init__()
        if len(critics) != 2:
            raise NotImplementedError(f"MOBILEPolicy: the HIP engine runs exactly two critics (run_mobile.py's --num-q-ensemble default), "
                                      f"got {len(critics)}")
        self.dynamics = dynamics
        self.actor = actor
        self.critics = critics
        self.critics_old = clone_target(critics)
        self.actor_optim, self.critics_optim = actor_optim, critics_optim
        self._tau, self._gamma = tau, gamma
        self._init_alpha(alpha)
        self._penalty_coef = penalty_coef
        self._num_samples = int(num_samples)
        self._deteterministic_backup = deterministic_backup
        self._layout = None            # (real rows, elites) of the bound engine

    def set_engine_options(self, n_runs=None, seed=None, precision=None, run_init=None):
        if n_runs is not None and n_runs > 1:
            raise NotImplementedError("MOBILEPolicy trains one run per policy object: n_runs > 1 is not supported (the penalty pairs ONE "
                                      "actor / critic pair with one dynamics ensemble)")
        return super().set_engine_options(n_runs=n_runs, seed=seed, precision=precision, run_init=run_init)

    @property
    def learn_n(self):
        raise AttributeError("MOBILEPolicy has no learn_n: every step needs the dynamics' next-state samples of its own batch "
                             "(learn({'real': ..., 'fake': ...}) / MBPolicyTrainer(fused=False))")

    def _nets(self):
        return {_engine.NET_ACTOR: self.actor, _engine.NET_CRITIC1: self.critics[0], _engine.NET_CRITIC2: self.critics[1],
                _engine.NET_CRITIC1_OLD: self.critics_old[0], _engine.NET_CRITIC2_OLD: self.critics_old[1]}

    def _optims(self):
        o = super()._optims()
        o[_engine.OPT_CRITIC] = self.critics_optim
        return o

    def _num_elites(self) -> int:
        return int(len(self.dynamics.model.elites))

    def _config(self) -> Dict:
        od, hid = _backbone_dims(self.actor.backbone)
        ad = self.actor.dist_net.mu.out_features
        self._check_dist_net()
        for c in self.critics:
            cin, chid = _backbone_dims(c.backbone)
            if chid != hid or cin != od + ad:
                raise NotImplementedError("MOBILE engine expects actor and critics to share hidden dims")
        real_rows, elites = self._layout if self._layout is not None else (0, self._num_elites())
        c = dict(obs_dim=od, act_dim=ad, hidden=hid, gamma=self._gamma, tau=self._tau,
                 actor_lr=float(self.actor_optim.param_groups[0]["lr"]), critic_lr=float(self.critics_optim.param_groups[0]["lr"]),
                 penalty_coef=float(self._penalty_coef), mobile_num_samples=self._num_samples, mobile_num_elites=int(elites),
                 mobile_real_rows=int(real_rows), deterministic_backup=int(bool(self._deteterministic_backup)))
        c.update(self._alpha_config())
        return c

    def _bind_layout(self, batch_size: int, real_rows: Optional[int]) -> None:
        """the real-row count and the elite count are part of the engine's row layout: a change rebuilds the engine around the current
        weights and optimizer state, as a batch-size change does"""
        if int(getattr(self.dynamics, "_n_runs", 1)) != 1 or self._n_runs != 1:
            raise NotImplementedError("MOBILEPolicy: one run per policy and per dynamics ensemble (n_runs == 1)")
        rows = real_rows if real_rows is not None else (self._layout[0] if self._layout is not None else 0)
        layout = (min(int(rows), int(batch_size)), self._num_elites())
        if layout != self._layout and self._eng is not None:
            carried = self._unbind()
            self._layout = layout
            self._rebind_with(carried, batch_size)
        else:
            self._layout = layout
            self._bind(batch_size)

    def _hand_over_samples(self, obss, actions, dyn_noise) -> torch.Tensor:
        dev = self._arena.device
        o = torch.as_tensor(obss, dtype=torch.float32, device=dev)
        a = torch.as_tensor(actions, dtype=torch.float32, device=dev)
        samples = self.dynamics.sample_next_obss_device(o, a, self._num_samples, noise=dyn_noise)
        if samples.device != dev:
            raise RuntimeError(f"MOBILEPolicy: the dynamics lives on {samples.device}, the policy engine on {dev}")
        samples = samples.contiguous()
        self._eng.set_next_samples(samples.data_ptr(), on_device=True)
        return samples          # (the engine borrows the memory until its next step: the caller keeps this alive)

    def compute_lcb(self, obss, actions, noise: Optional[Sequence] = None) -> torch.Tensor:
        """mobile.py:130-142: the (B, 1) penalty -- std over the elites of the mean over ``num_samples`` draws of min Q_old(s', pi(s')) --
        through the device path ``learn`` uses, without the zeroing of the real rows.  ``noise`` = (eps_lcb (S*E*B, act_dim), dynamics
        noise (S, E, B, obs_dim + 1)) teacher-forces the draws."""
        B = int(np.shape(obss)[-2])
        self._bind_layout(B, None)
        eps, dyn_noise = (noise[0], noise[1]) if noise is not None else (None, None)
        dev = self._arena.device
        keep = self._hand_over_samples(obss, actions, dyn_noise)
        out = torch.empty((1, B), dtype=torch.float32, device=dev)
        e = None if eps is None else torch.as_tensor(eps, dtype=torch.float32, device=dev).reshape(1, -1, self.actor.dist_net.mu.out_features).contiguous()
        torch.cuda.current_stream(dev).synchronize()
        self._eng.lcb_penalty(None if e is None else e.data_ptr(), out.data_ptr(), on_device=True)
        del keep
        return out.reshape(B, 1)

    def learn(self, batch: Dict, noise: Optional[Sequence] = None) -> Dict[str, float]:
        """mobile.py:144-196 on ``{"real": batch, "fake": batch}``.  ``noise`` = [eps_lcb (S*E*B, A), eps_next (B, A), eps_actor (B, A),
        dynamics noise (S, E, B, obs_dim + 1)]: the three engine slots in the reference's draw order plus the ``randn_like`` draws of
        ``sample_next_obss``."""
        if "real" not in batch:
            raise ValueError("MOBILEPolicy.learn expects {'real': batch, 'fake': batch} (mobile.py:145-146)")
        real_rows = int(batch["real"]["observations"].shape[-2])
        mix = _cat(batch)
        if np.ndim(mix["observations"]) != 2:
            raise ValueError("MOBILEPolicy.learn: [B, cols] batches (one run per policy)")
        self._bind_layout(int(mix["observations"].shape[0]), real_rows)
        eng_noise, dyn_noise = (list(noise[:3]), noise[3]) if noise is not None else (None, None)
        keep = self._hand_over_samples(mix["observations"], mix["actions"], dyn_noise)
        out = super().learn(mix, eng_noise)
        del keep
        return out

    def rollout(self, init_obss: np.ndarray, rollout_length: int):
        return _rollout(self, init_obss, rollout_length, False)


class MOBILEDevicePolicy(MOBILEPolicy):
    """``MOBILEPolicy`` with the fused epoch of ``MBPolicyTrainer(fused=True)``: same constructor, ``state_dict``, ``learn``,
    ``compute_lcb`` and ``rollout``; ``learn_n`` runs whole steps as one device loop (``orl_mobile_learn_n``) and ``rollout_device`` is
    MOPO's device rollout (the reference's ``MOBILEPolicy.rollout`` is the same loop as MOPO's).  One run per policy, one model ring."""

    def _one_ring(self, fake_buffer, what: str) -> None:
        if isinstance(fake_buffer, (list, tuple)):
            raise NotImplementedError(f"MOBILEDevicePolicy.{what}: one model ring (a sequence of per-run rings needs n_runs > 1, and "
                                      "MOBILE trains one run per policy object)")
        if int(getattr(self.dynamics, "_n_runs", 1)) != 1 or self._n_runs != 1:
            raise NotImplementedError(f"MOBILEDevicePolicy.{what}: one run per policy and per dynamics ensemble (n_runs == 1)")

    def rollout_device(self, real_buffer, fake_buffer, rollout_batch_size: int, rollout_length: int, init_obss=None) -> Dict:
        """``rollout`` + ``fake_buffer.add_batch`` on the device (``MOPOPolicy.rollout_device``); returns the reference's rollout info"""
        self._one_ring(fake_buffer, "rollout_device")
        return _rollout_device_any(self, real_buffer, fake_buffer, rollout_batch_size, rollout_length, init_obss, False)

    def learn_n(self, n_steps: int, real_buffer, fake_buffer=None, batch_size: int = 256, real_ratio: float = 0.05) -> Dict[str, float]:
        """the inner loop of MBPolicyTrainer (mb_policy_trainer.py:78-90) as one device loop: rows [0, int(batch_size * real_ratio)) of
        every minibatch from ``real_buffer``, the rest from ``fake_buffer``'s ring, the dynamics' next-state samples of the drawn rows
        written straight into the penalty pass's operands; returns the per-key means"""
        if real_buffer is None or fake_buffer is None:
            raise NotImplementedError("MOBILEDevicePolicy mixes a real and a model-rollout buffer per batch: "
                                      "learn_n(n_steps, real_buffer, fake_buffer, ...), or learn({'real': ..., 'fake': ...})")
        self._one_ring(fake_buffer, "learn_n")
        real_rows = int(batch_size * real_ratio)               # mb_policy_trainer.py:81-82
        self._bind_layout(int(batch_size), real_rows)
        real = real_buffer.device_buffer() if hasattr(real_buffer, "device_buffer") else real_buffer
        model = fake_buffer.reserve_device() if hasattr(fake_buffer, "reserve_device") else fake_buffer
        key = (real, model, real_rows)
        if self._attached != key:
            self._eng.attach_buffer(real)
            self._eng.attach_model_buffer(model, real_rows)
            self._attached = key
        self._push_lrs()
        dyn, _, _ = self.dynamics.loop_engine()
        m, ms = self._eng.mobile_learn_n(dyn, int(n_steps))
        self.last_learn_n_ms = ms
        return self._result(m)

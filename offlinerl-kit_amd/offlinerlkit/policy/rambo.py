"""RAMBO (reference: policy/model_based/rambo.py:16-248): MOPO's SAC update on the HIP engine plus the adversarial update of the dynamics
ensemble during policy learning.

``update_dynamics`` keeps the reference's host loop and buffer draws.  One ``dynamics_step_and_forward`` is two calls into the dynamics
engine (``EnsembleDynamics.adv_forward_device`` / ``adv_update_device``, ``orl_dynadv_*``): the ensemble forward over the rollout and
the dataset rows with the sample, then the mixture log-probability, the advantage-weighted policy-gradient term, the Gaussian NLL, one
backward and one Adam step of ``dynamics_adv_optim``.  Between them the advantage is computed from the policy's torch views of the actor
and the critics (the engine's live weights) under ``no_grad``; the termination function runs on the host like the reference's.
``pretrain`` (behaviour cloning of the actor, once) is plain torch autograd on the same views.

``update_dynamics_device`` is the same update as ONE call into the device loop (``orl_rambo_update_dynamics``): the actor's draws, the
buffer draws (device Philox instead of numpy's), the adversarial forward, the advantage on the policy engine
(``orl_engine_adv_advantage``'s pass: termination test, TD value and normalisation in one kernel) and the adversarial update of every
step are enqueued on one stream, and the five logged values are read once at the end.  ``MBPolicyTrainer(fused=True,
dynamics_update_freq > 0)`` calls it; ``rambo_adv_schedule`` is the reference loop's segment structure as a pure function.

One run per policy: ``set_engine_options(n_runs > 1)`` is refused (the calls underneath are run-batched).
"""
from __future__ import annotations

import os
from collections import defaultdict
from typing import Dict, List, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from .model_based import MOPOPolicy

_KEYS = ("all_loss", "sl_loss", "adv_loss", "adv_advantage", "adv_log_prob")


def rambo_adv_schedule(adv_train_steps: int, rollout_length: int) -> List[int]:
    """The segment lengths of ``update_dynamics``' loop (rambo.py:101-125): ``while steps < adv_train_steps`` draws initial states, the
    ``for`` over ``rollout_length`` steps them, and ``if steps == 1000: break`` leaves the ``for`` -- at the literal 1000, whatever
    ``adv_train_steps`` is, and the ``while`` then starts a new segment if steps are still missing.  The ``for`` is not left when
    ``adv_train_steps`` is reached, so the total overshoots to the end of the segment.  A pure function of its two arguments."""
    if rollout_length < 1:
        raise ValueError("rollout_length must be >= 1")
    segments, steps = [], 0
    while steps < adv_train_steps:
        n = 0
        for _ in range(rollout_length):
            n += 1
            steps += 1
            if steps == 1000:
                break
        segments.append(n)
    return segments


class RAMBOPolicy(MOPOPolicy):
    """RAMBO-RL: Robust Adversarial Model-Based Offline Reinforcement Learning <Ref: https://arxiv.org/abs/2204.12581>;
    constructor = rambo.py:21-62."""

    def __init__(self, dynamics, actor: nn.Module, critic1: nn.Module, critic2: nn.Module, actor_optim, critic1_optim, critic2_optim,
                 dynamics_adv_optim, tau: float = 0.005, gamma: float = 0.99, alpha: Union[float, Tuple] = 0.2, adv_weight: float = 0,
                 adv_train_steps: int = 1000, adv_rollout_batch_size: int = 256, adv_rollout_length: int = 5,
                 include_ent_in_adv: bool = False, scaler=None, device="cpu") -> None:
        super().__init__(dynamics, actor, critic1, critic2, actor_optim, critic1_optim, critic2_optim, tau=tau, gamma=gamma, alpha=alpha)
        self._dynmics_adv_optim = dynamics_adv_optim
        self._adv_weight = adv_weight
        self._adv_train_steps = adv_train_steps
        self._adv_rollout_batch_size = adv_rollout_batch_size
        self._adv_rollout_length = adv_rollout_length
        self._include_ent_in_adv = include_ent_in_adv
        self.scaler = scaler
        self.device = device

    def set_engine_options(self, n_runs=None, seed=None, precision=None, run_init=None):
        if n_runs is not None and n_runs > 1:
            raise NotImplementedError("RAMBOPolicy trains one run per policy object: n_runs > 1 is not supported (the adversarial "
                                      "dynamics update pairs ONE actor / critic pair with one ensemble)")
        return super().set_engine_options(n_runs=n_runs, seed=seed, precision=precision, run_init=run_init)

    def load(self, path: str) -> None:
        self.load_state_dict(torch.load(os.path.join(path, "rambo_pretrain.pth"), map_location=self._torch_device()))

    def _torch_device(self) -> torch.device:
        return next(self.actor.parameters()).device

    def pretrain(self, data: Dict, n_epoch: int, batch_size: int, lr: float, logger) -> None:
        """rambo.py:67-93: behaviour cloning of the actor with torch autograd (the parameters are the engine's live weights once it is
        bound), ``rambo_pretrain.pth`` in ``logger.model_dir``.  The per-epoch mean losses are kept in ``pretrain_losses``."""
        self._bc_optim = torch.optim.Adam(self.actor.parameters(), lr=lr)
        observations = data["observations"]
        actions = data["actions"]
        sample_num = observations.shape[0]
        idxs = np.arange(sample_num)
        dev = self._torch_device()
        logger.log("Pretraining policy")
        self.actor.train()
        self.pretrain_losses = []
        for i_epoch in range(n_epoch):
            np.random.shuffle(idxs)
            sum_loss, n_batch = 0.0, sample_num // batch_size
            for i_batch in range(n_batch):
                batch_obs = torch.from_numpy(np.asarray(observations[i_batch * batch_size: (i_batch + 1) * batch_size], np.float32)).to(dev)
                batch_act = torch.from_numpy(np.asarray(actions[i_batch * batch_size: (i_batch + 1) * batch_size], np.float32)).to(dev)
                dist = self.actor(batch_obs)
                pred_actions, _ = dist.rsample()
                bc_loss = ((pred_actions - batch_act) ** 2).mean()
                self._bc_optim.zero_grad()
                bc_loss.backward()
                self._bc_optim.step()
                sum_loss += bc_loss.cpu().item()
            self.pretrain_losses.append(sum_loss / max(n_batch, 1))
            logger.log(f"Epoch {i_epoch}, mean bc loss {self.pretrain_losses[-1]}")
        sd = self.state_dict()
        torch.save(type(sd)((k, v.detach().clone()) for k, v in sd.items()), os.path.join(logger.model_dir, "rambo_pretrain.pth"))

    def update_dynamics(self, real_buffer) -> Dict[str, float]:
        """rambo.py:95-127: the buffer draws in the reference's order, ``adv_train_steps`` model updates (and its ``steps == 1000`` break)"""
        if int(getattr(self.dynamics, "_n_runs", 1)) != 1 or self._n_runs != 1:
            raise NotImplementedError("RAMBOPolicy.update_dynamics: one run per policy and per dynamics ensemble (n_runs == 1)")
        all_loss_info = {"adv_dynamics_update/" + k: 0 for k in _KEYS}
        self.dynamics.model.train()
        steps = 0
        while steps < self._adv_train_steps:
            init_obss = real_buffer.sample(self._adv_rollout_batch_size)["observations"].cpu().numpy()
            observations = init_obss
            for t in range(self._adv_rollout_length):
                actions = MOPOPolicy.select_action(self, observations)
                batch = real_buffer.sample(self._adv_rollout_batch_size)
                next_observations, terminals, loss_info = self.dynamics_step_and_forward(
                    observations, actions, batch["observations"], batch["actions"], batch["next_observations"], batch["rewards"])
                for _key in loss_info:
                    all_loss_info[_key] += loss_info[_key]
                steps += 1
                observations = next_observations.copy()
                if steps == 1000:
                    break
        self.dynamics.model.eval()
        return {_key: _value / steps for _key, _value in all_loss_info.items()}

    def update_dynamics_device(self, real_buffer) -> Dict[str, float]:
        """``update_dynamics`` as ONE call into the device loop (``orl_rambo_update_dynamics``): the actor's draws, the buffer draws,
        the adversarial forward, the advantage on the engine and the adversarial update of every step are enqueued without a host
        round trip, and the five values are read once.  The draws come from the device Philox streams (the buffer's, the dynamics' and
        the loop's own for the actions) instead of numpy's and torch's: reproducible from the seeds, not index-identical to
        ``update_dynamics``.  ``last_update_dynamics_ms`` holds the HIP-event time of the loop."""
        dyn = self.dynamics
        if int(getattr(dyn, "_n_runs", 1)) != 1 or self._n_runs != 1:
            raise NotImplementedError("RAMBOPolicy.update_dynamics_device: one run per policy and per dynamics ensemble (n_runs == 1)")
        kind = getattr(dyn, "term_kind", None)
        if kind is None:
            raise NotImplementedError("rollout_device: the dynamics' termination function is not one of the fixed row-wise tests of "
                                      "utils.termination_fns (an obs_unnormalization wrapper, door or another callable carries no term_kind): "
                                      "the device rollout cannot evaluate it; use rollout() / MBPolicyTrainer(fused=False)")
        if not hasattr(real_buffer, "device_buffer"):
            raise NotImplementedError("RAMBOPolicy.update_dynamics_device: the buffer has no device_buffer() (an HBM-resident "
                                      "offlinerlkit.buffer.ReplayBuffer is needed); use update_dynamics()")
        rows = int(self._adv_rollout_batch_size)
        if self._eng is None:
            self._bind(256)
        dyn.bind_adversary(self._dynmics_adv_optim, self._adv_weight, rows, rows)
        dyn._adv_ready()
        real = real_buffer.device_buffer()
        dyn.model.train()
        torch.cuda.current_stream(self._torch_device()).synchronize()
        try:
            m, ms = self._eng.rambo_update_dynamics(dyn._eng, real, rows, int(kind), bool(self._include_ent_in_adv),
                                                    rambo_adv_schedule(self._adv_train_steps, self._adv_rollout_length))
        finally:
            dyn.model.eval()
        self.last_update_dynamics_ms = ms
        return {"adv_dynamics_update/" + k: m[k] for k in _KEYS}

    def dynamics_step_and_forward(self, observations, actions, sl_observations, sl_actions, sl_next_observations, sl_rewards):
        """rambo.py:129-207 -> (next_observations, terminals, the five ``adv_dynamics_update/*`` values)"""
        dyn = self.dynamics
        observations = np.asarray(observations, np.float32)
        actions = np.asarray(actions, np.float32)
        dyn.bind_adversary(self._dynmics_adv_optim, self._adv_weight, len(observations), int(sl_observations.shape[0]))
        nxt, rew = dyn.adv_forward_device(observations, actions, sl_observations, sl_actions, sl_next_observations, sl_rewards)
        next_observations = nxt.cpu().numpy()
        terminals = dyn.terminal_fn(observations, actions, next_observations)
        with torch.no_grad():
            dev = next(self.critic1.parameters()).device
            obs_t, act_t = torch.as_tensor(observations, device=dev), torch.as_tensor(actions, device=dev)
            nxt_t, rew_t = nxt.to(dev), rew.to(dev).unsqueeze(-1)
            next_actions, next_policy_log_prob = self.actforward(nxt_t, deterministic=True)
            next_q = torch.minimum(self.critic1(nxt_t, next_actions), self.critic2(nxt_t, next_actions))
            if self._include_ent_in_adv:
                next_q = next_q - self._alpha * next_policy_log_prob
            value = rew_t + (1 - torch.as_tensor(np.asarray(terminals), device=dev).float().reshape(-1, 1)) * self._gamma * next_q
            value_baseline = torch.minimum(self.critic1(obs_t, act_t), self.critic2(obs_t, act_t))
            advantage = value - value_baseline
            advantage = (advantage - advantage.mean()) / (advantage.std() + 1e-6)
            adv_mean = advantage.mean().cpu().item()
        m = dyn.adv_update_device(advantage.reshape(-1))
        return next_observations, terminals, {
            "adv_dynamics_update/all_loss": m["all_loss"],
            "adv_dynamics_update/sl_loss": m["sl_loss"],
            "adv_dynamics_update/adv_loss": m["adv_loss"],
            "adv_dynamics_update/adv_advantage": adv_mean,
            "adv_dynamics_update/adv_log_prob": m["adv_log_prob"],
        }

    def rollout(self, init_obss: np.ndarray, rollout_length: int) -> Tuple[Dict[str, np.ndarray], Dict]:
        """rambo.py:209-243: MOPO's rollout with the actions of the UNSCALED observations (the reference calls super().select_action)"""
        num_transitions = 0
        rewards_arr = np.array([])
        out = defaultdict(list)
        observations = init_obss
        for _ in range(rollout_length):
            actions = MOPOPolicy.select_action(self, observations)
            next_observations, rewards, terminals, info = self.dynamics.step(observations, actions)
            out["obss"].append(observations); out["next_obss"].append(next_observations); out["actions"].append(actions)
            out["rewards"].append(rewards); out["terminals"].append(terminals)
            num_transitions += len(observations)
            rewards_arr = np.append(rewards_arr, rewards.flatten())
            nonterm_mask = (~terminals).flatten()
            if nonterm_mask.sum() == 0:
                break
            observations = next_observations[nonterm_mask]
        return {k: np.concatenate(v, axis=0) for k, v in out.items()}, {"num_transitions": num_transitions, "reward_mean": rewards_arr.mean()}

    def select_action(self, obs: np.ndarray, deterministic: bool = False) -> np.ndarray:
        if self.scaler is not None:
            obs = self.scaler.transform(obs)
        return super().select_action(obs, deterministic)

"""SAC and the model-based callers of the hot path (reference: policy/model_free/sac.py:11-140, policy/model_based/mopo.py:14-84,
policy/model_based/combo.py:12-241) on the HIP engine.

``MOPOPolicy.learn`` and ``COMBOPolicy.learn`` take ``{"real": batch, "fake": batch}``, concatenate real rows first and run the SAC /
CQL-variant update of the engine on the mixed batch.  ``rollout`` needs an object with ``step(obs, act) -> (next_obs, reward, terminal,
info)``: ``offlinerlkit.dynamics.EnsembleDynamics`` with a function of ``utils.termination_fns``.  ``policy_trainer.MBPolicyTrainer`` runs
the reference's loop around them.

The fused epoch (``MBPolicyTrainer(fused=True)``) keeps the model buffer in an HBM ring (``ReplayBuffer.reserve_device``):
``rollout_device`` rolls the dynamics forward without a host round trip (``EnsembleDynamics.step_device`` and the termination /
compaction kernel behind ``DeviceBuffer.append_rollout``) and ``learn_n(n_steps, real_buffer, fake_buffer, ...)`` draws the real and
the model rows of every minibatch inside ``orl_learn_n`` (``orl_engine_attach_model_buffer``).

Per-run model rings: where ``fake_buffer`` is a sequence of ``n_runs`` ``ReplayBuffer``s (instead of one), run r of a multi-run policy
rolls ITS actor through run r of the dynamics (or a shared one-run ensemble) into ring r and draws its model rows from ring r only --
R independent seeds.  All runs share the launches: one batched actor forward (``actforward_runs``), one ``step_device_runs``, one
``DeviceBuffer.append_rollout_runs`` per model step, and ``orl_engine_attach_model_buffers`` for ``learn_n``.  One ``ReplayBuffer``
keeps the single shared ring, filled by the selected run's actor.
"""
from __future__ import annotations

from collections import defaultdict
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from .. import _engine
from .base_policy import _backbone_dims, clone_target
from .sac_family import CQLPolicy, _TanhGaussPolicy


def _cat(batch: Dict) -> Dict:
    """real rows first, then model rows (mopo.py:81-84 / combo.py:111-113); with a leading run dimension ([R, B, cols] arrays of a
    multi-run policy) the ROW axis is the second to last one"""
    real, fake = batch["real"], batch["fake"]
    out = {}
    for k in real:
        a, b = real[k], fake[k]
        if np.ndim(a) != np.ndim(b) or np.ndim(a) < 2:
            raise ValueError(f"{k}: real batch has shape {tuple(np.shape(a))}, model batch {tuple(np.shape(b))}: both must be [B, cols] or [R, B, cols]")
        out[k] = torch.cat([torch.as_tensor(a), torch.as_tensor(b).to(torch.as_tensor(a).device)], -2) if torch.is_tensor(a) or torch.is_tensor(b) \
            else np.concatenate([np.asarray(a), np.asarray(b)], -2)
    return out


def _rollout(policy, init_obss: np.ndarray, rollout_length: int, uniform: bool) -> Tuple[Dict[str, np.ndarray], Dict]:
    """mopo.py:43-79 / combo.py:67-108: roll the learned dynamics forward from dataset states under the current policy."""
    num_transitions = 0
    rewards_arr = np.array([])
    out = defaultdict(list)
    observations = init_obss
    for _ in range(rollout_length):
        if uniform:
            sp = policy.action_space
            actions = np.random.uniform(sp.low[0], sp.high[0], size=(len(observations), sp.shape[0]))
        else:
            actions = policy.select_action(observations)
        next_observations, rewards, terminals, info = policy.dynamics.step(observations, actions)
        out["obss"].append(observations); out["next_obss"].append(next_observations); out["actions"].append(actions)
        out["rewards"].append(rewards); out["terminals"].append(terminals)
        num_transitions += len(observations)
        rewards_arr = np.append(rewards_arr, rewards.flatten())
        nonterm = (~terminals).flatten()
        if nonterm.sum() == 0:
            break
        observations = next_observations[nonterm]
    return {k: np.concatenate(v, axis=0) for k, v in out.items()}, {"num_transitions": num_transitions, "reward_mean": rewards_arr.mean()}


def _rollout_device(policy, real_buffer, fake_buffer, rollout_batch_size: int, rollout_length: int, init_obss, uniform: bool) -> Dict:
    """``_rollout`` with every array on the device: the transitions go straight into ``fake_buffer``'s HBM ring.  One host sync per
    model step (the count of surviving rows sizes the next step).  The compaction keeps the surviving rows in their order, so the
    dynamics consumes the Philox draws the host rollout consumes."""
    dyn = policy.dynamics
    kind = getattr(dyn, "term_kind", None)
    if kind is None or not hasattr(dyn, "step_device"):
        raise NotImplementedError("rollout_device: the dynamics' termination function is not one of the fixed row-wise tests of "
                                  "utils.termination_fns (an obs_unnormalization wrapper, door or another callable carries no term_kind): "
                                  "the device rollout cannot evaluate it; use rollout() / MBPolicyTrainer(fused=False)")
    ring = fake_buffer.reserve_device()
    if init_obss is None:
        init_obss = real_buffer.sample(rollout_batch_size)["observations"]
    dev = torch.device("cuda", ring.device)
    obs = torch.as_tensor(init_obss, dtype=torch.float32, device=dev).reshape(len(init_obss), -1).contiguous()
    num_transitions, rew_sum = 0, 0.0
    with torch.no_grad():
        for _ in range(rollout_length):
            n = int(obs.shape[0])
            if uniform:
                sp = policy.action_space
                act = torch.empty((n, sp.shape[0]), dtype=torch.float32, device=dev).uniform_(float(sp.low[0]), float(sp.high[0]))
            else:
                act, _ = policy.actforward(obs, False)
                act = act.to(torch.float32).contiguous()
            nxt, rew, _ = dyn.step_device(obs, act)
            alive = torch.empty_like(nxt)
            n_alive, s = ring.append_rollout(kind, obs, act, nxt.contiguous(), rew.contiguous(), alive)
            fake_buffer._advance(n)
            num_transitions += n
            rew_sum += s
            if n_alive == 0:
                break
            obs = alive[:n_alive]
    return {"num_transitions": num_transitions, "reward_mean": rew_sum / num_transitions}


def per_run_rings(policy, fake_buffer) -> Optional[List]:
    """``fake_buffer`` given as a sequence -> the list of the runs' buffers (checked: one per run, same dims, capacity and device);
    a single buffer -> None"""
    if not isinstance(fake_buffer, (list, tuple)):
        return None
    bufs = list(fake_buffer)
    R = int(getattr(policy, "n_runs", 1))
    if len(bufs) != R:
        raise ValueError(f"per-run model buffers: {len(bufs)} buffers for a policy of n_runs = {R} (one ring per run)")
    if len({id(b) for b in bufs}) != R:
        raise ValueError("per-run model buffers: the same buffer is listed twice (one ring per run)")
    shape = lambda b: (tuple(b.obs_shape), int(b.action_dim), int(b._max_size), str(b.device))
    for r, b in enumerate(bufs):
        if shape(b) != shape(bufs[0]):
            raise ValueError(f"per-run model buffers: run {r}'s buffer (obs shape, action dim, capacity, device) = {shape(b)} differs "
                             f"from run 0's {shape(bufs[0])}")
    return bufs


def _rollout_device_runs(policy, real_buffer, bufs, rollout_batch_size: int, rollout_length: int, init_obss, uniform: bool) -> Dict:
    """``_rollout_device`` for the R runs of a policy at once, run r into ``bufs[r]``: one batched actor forward, one dynamics step
    and one termination / compaction launch pair per model step for all runs.  The runs' live row counts diverge; every step runs at
    the largest one, with zeroed padding rows behind a run's live rows (finite inputs, ignored outputs).  One host sync per model step."""
    dyn = policy.dynamics
    kind = getattr(dyn, "term_kind", None)
    if kind is None or not hasattr(dyn, "step_device_runs"):
        raise NotImplementedError("rollout_device: the dynamics' termination function is not one of the fixed row-wise tests of "
                                  "utils.termination_fns (an obs_unnormalization wrapper, door or another callable carries no term_kind): "
                                  "the device rollout cannot evaluate it; use rollout() / MBPolicyTrainer(fused=False)")
    R, N = len(bufs), int(rollout_batch_size)
    if int(getattr(dyn, "_n_runs", 1)) not in (1, R):
        raise ValueError(f"per-run model buffers: the dynamics carries {dyn._n_runs} runs; {R} (run r rolls through ensemble r) or 1 (shared)")
    rings = [b.reserve_device() for b in bufs]
    if init_obss is None:
        init_obss = real_buffer.sample(R * N)["observations"]
    dev = torch.device("cuda", rings[0].device)
    obs = torch.as_tensor(init_obss, dtype=torch.float32, device=dev).reshape(R, N, -1).contiguous()
    if not uniform and policy._eng is None:
        policy._bind(256)                      # (the stacked actor tensors live in the engine's arena)
    live = np.full(R, N, dtype=np.int64)
    num_transitions, rew_sum = np.zeros(R, np.int64), np.zeros(R, np.float64)
    with torch.no_grad():
        for _ in range(rollout_length):
            nmax = int(live.max())
            obs = obs[:, :nmax].contiguous()
            if uniform:
                sp = policy.action_space
                act = torch.empty((R, nmax, sp.shape[0]), dtype=torch.float32, device=dev).uniform_(float(sp.low[0]), float(sp.high[0]))
            else:
                act = policy.actforward_runs(obs, False).contiguous()
            nxt, rew, _ = dyn.step_device_runs(obs, act)
            alive = torch.zeros_like(nxt)      # zeros: the rows past a run's survivors are the next step's padding
            n_alive, s = _engine.DeviceBuffer.append_rollout_runs(rings, kind, obs, act, nxt.contiguous(), rew.contiguous(), live, alive)
            for r in range(R):
                if live[r]:
                    bufs[r]._advance(int(live[r]))
            num_transitions += live
            rew_sum += s
            live = n_alive
            if int(live.max()) == 0:
                break
            obs = alive
    return {"num_transitions": num_transitions, "reward_mean": rew_sum / np.maximum(num_transitions, 1)}


def _rollout_device_any(policy, real_buffer, fake_buffer, rollout_batch_size: int, rollout_length: int, init_obss, uniform: bool) -> Dict:
    bufs = per_run_rings(policy, fake_buffer)
    if bufs is None:
        return _rollout_device(policy, real_buffer, fake_buffer, rollout_batch_size, rollout_length, init_obss, uniform)
    return _rollout_device_runs(policy, real_buffer, bufs, rollout_batch_size, rollout_length, init_obss, uniform)


def _learn_n_mb(policy, n_steps: int, real_buffer, fake_buffer, batch_size: int, real_ratio: float) -> Dict[str, float]:
    """``n_steps`` x (sample real, sample model, learn) fused on the device: both index draws inside ``orl_learn_n``.  A sequence of
    buffers as ``fake_buffer``: run r's model rows from ring r (``orl_engine_attach_model_buffers``)."""
    if real_buffer is None or fake_buffer is None:
        raise NotImplementedError(f"{type(policy).__name__} mixes a real and a model-rollout buffer per batch: "
                                  "learn_n(n_steps, real_buffer, fake_buffer, ...), or learn({'real': ..., 'fake': ...})")
    bufs = per_run_rings(policy, fake_buffer)
    real_rows = int(batch_size * real_ratio)               # mb_policy_trainer.py:81-82
    policy._bind(batch_size)
    real = real_buffer.device_buffer() if hasattr(real_buffer, "device_buffer") else real_buffer
    if bufs is not None:
        models = tuple(b.reserve_device() for b in bufs)
        key = (real, models, real_rows)
    else:
        model = fake_buffer.reserve_device() if hasattr(fake_buffer, "reserve_device") else fake_buffer
        key = (real, model, real_rows)
    if policy._attached != key:
        policy._eng.attach_buffer(real)
        if bufs is not None:
            policy._eng.attach_model_buffers(models, real_rows)
        else:
            policy._eng.attach_model_buffer(model, real_rows)
        policy._attached = key
    policy._push_lrs()
    m, ms = policy._eng.learn_n(int(n_steps))
    policy.last_learn_n_ms = ms
    return policy._result(m)


class SACPolicy(_TanhGaussPolicy):
    """Soft Actor-Critic; constructor = reference SACPolicy.__init__ (sac.py:16-48)."""

    ALGO = "sac"

    def __init__(self, actor: nn.Module, critic1: nn.Module, critic2: nn.Module, actor_optim, critic1_optim, critic2_optim,
                 tau: float = 0.005, gamma: float = 0.99, alpha: Union[float, Tuple] = 0.2) -> None:
        super().__init__()
        self.actor = actor
        self.critic1, self.critic1_old = critic1, clone_target(critic1)
        self.critic2, self.critic2_old = critic2, clone_target(critic2)
        self.actor_optim, self.critic1_optim, self.critic2_optim = actor_optim, critic1_optim, critic2_optim
        self._tau, self._gamma = tau, gamma
        self._init_alpha(alpha)
        if float(critic1_optim.param_groups[0]["lr"]) != float(critic2_optim.param_groups[0]["lr"]):
            raise NotImplementedError("critic1/critic2 must share a learning rate")

    def _nets(self):
        return {_engine.NET_ACTOR: self.actor, _engine.NET_CRITIC1: self.critic1, _engine.NET_CRITIC2: self.critic2,
                _engine.NET_CRITIC1_OLD: self.critic1_old, _engine.NET_CRITIC2_OLD: self.critic2_old}

    def _optims(self):
        o = super()._optims()
        o[_engine.OPT_CRITIC] = self.critic1_optim
        return o

    def _config(self) -> Dict:
        od, hid = _backbone_dims(self.actor.backbone)
        cin, chid = _backbone_dims(self.critic1.backbone)
        ad = self.actor.dist_net.mu.out_features
        self._check_dist_net()
        if chid != hid or cin != od + ad:
            raise NotImplementedError("SAC engine expects actor and critics to share hidden dims")
        c = dict(obs_dim=od, act_dim=ad, hidden=hid, gamma=self._gamma, tau=self._tau,
                 actor_lr=float(self.actor_optim.param_groups[0]["lr"]), critic_lr=float(self.critic1_optim.param_groups[0]["lr"]))
        c.update(self._alpha_config())
        return c


class MOPOPolicy(SACPolicy):
    """Model-based Offline Policy Optimization <Ref: https://arxiv.org/abs/2005.13239>; constructor = mopo.py:19-41."""

    def __init__(self, dynamics, actor, critic1, critic2, actor_optim, critic1_optim, critic2_optim, tau: float = 0.005,
                 gamma: float = 0.99, alpha: Union[float, Tuple] = 0.2) -> None:
        super().__init__(actor, critic1, critic2, actor_optim, critic1_optim, critic2_optim, tau=tau, gamma=gamma, alpha=alpha)
        self.dynamics = dynamics

    def rollout(self, init_obss: np.ndarray, rollout_length: int):
        return _rollout(self, init_obss, rollout_length, False)

    def learn(self, batch: Dict, noise=None) -> Dict[str, float]:
        return super().learn(_cat(batch), noise) if "real" in batch else super().learn(batch, noise)

    def rollout_device(self, real_buffer, fake_buffer, rollout_batch_size: int, rollout_length: int, init_obss=None) -> Dict:
        """``rollout`` + ``fake_buffer.add_batch`` on the device; returns the reference's rollout info.  ``fake_buffer`` = a sequence of
        ``n_runs`` buffers: every run rolls its own actor into its own ring, ``rollout_batch_size`` initial states each, and the info
        holds per-run arrays ``num_transitions[R]`` / ``reward_mean[R]``"""
        return _rollout_device_any(self, real_buffer, fake_buffer, rollout_batch_size, rollout_length, init_obss, False)

    def learn_n(self, n_steps: int, real_buffer, fake_buffer=None, batch_size: int = 256, real_ratio: float = 0.05) -> Dict[str, float]:
        """the inner loop of MBPolicyTrainer (mb_policy_trainer.py:78-90) fused on the device: rows [0, int(batch_size * real_ratio))
        of every minibatch from ``real_buffer``, the rest from ``fake_buffer``'s ring; returns the per-key means.  The single-buffer
        form of the model-free policies is refused: every batch mixes a real and a model-rollout buffer."""
        return _learn_n_mb(self, n_steps, real_buffer, fake_buffer, batch_size, real_ratio)


class COMBOPolicy(CQLPolicy):
    """Conservative Offline Model-Based Policy Optimization <Ref: https://arxiv.org/abs/2102.08363>; constructor = combo.py:18-65."""

    def __init__(self, dynamics, actor, critic1, critic2, actor_optim, critic1_optim, critic2_optim, action_space, tau: float = 0.005,
                 gamma: float = 0.99, alpha: Union[float, Tuple] = 0.2, cql_weight: float = 1.0, temperature: float = 1.0,
                 max_q_backup: bool = False, deterministic_backup: bool = True, with_lagrange: bool = True,
                 lagrange_threshold: float = 10.0, cql_alpha_lr: float = 1e-4, num_repeart_actions: int = 10,
                 uniform_rollout: bool = False, rho_s: str = "mix") -> None:
        super().__init__(actor, critic1, critic2, actor_optim, critic1_optim, critic2_optim, action_space, tau=tau, gamma=gamma, alpha=alpha,
                         cql_weight=cql_weight, temperature=temperature, max_q_backup=max_q_backup, deterministic_backup=deterministic_backup,
                         with_lagrange=with_lagrange, lagrange_threshold=lagrange_threshold, cql_alpha_lr=cql_alpha_lr,
                         num_repeart_actions=num_repeart_actions)
        if rho_s not in ("model", "mix"):
            raise ValueError("rho_s must be 'model' or 'mix'")
        self.dynamics = dynamics
        self._uniform_rollout = uniform_rollout
        self._rho_s = rho_s
        self._rows = None          # (real rows, model rows) of the bound engine

    def rollout(self, init_obss: np.ndarray, rollout_length: int):
        return _rollout(self, init_obss, rollout_length, self._uniform_rollout)

    def _config(self) -> Dict:
        c = super()._config()
        if self._rows is not None:
            br, bf = self._rows
            c0, bc = (br, bf) if self._rho_s == "model" else (0, br + bf)
            c.update(cql_cons_row0=int(c0), cql_cons_rows=int(bc), cql_real_rows=int(br))
        return c

    def learn(self, batch: Dict, noise=None) -> Dict[str, float]:
        if "real" not in batch:
            raise ValueError("COMBOPolicy.learn expects {'real': batch, 'fake': batch} (combo.py:110-113)")
        rows = (int(batch["real"]["observations"].shape[-2]), int(batch["fake"]["observations"].shape[-2]))
        if rows != self._rows:
            if self._eng is not None:      # the real / model split is part of the engine's row layout: rebuild around the current state
                carried = self._unbind()
                self._rows = rows
                self._rebind_with(carried, rows[0] + rows[1])
            else:
                self._rows = rows
        return super().learn(_cat(batch), noise)

    def rollout_device(self, real_buffer, fake_buffer, rollout_batch_size: int, rollout_length: int, init_obss=None) -> Dict:
        """``rollout`` + ``fake_buffer.add_batch`` on the device (uniform actions from torch's device generator when ``uniform_rollout``)"""
        return _rollout_device_any(self, real_buffer, fake_buffer, rollout_batch_size, rollout_length, init_obss, self._uniform_rollout)

    def learn_n(self, n_steps: int, real_buffer, fake_buffer=None, batch_size: int = 256, real_ratio: float = 0.05) -> Dict[str, float]:
        """as ``MOPOPolicy.learn_n``; the real / model split is part of the engine's row layout, so a changed split re-binds"""
        if real_buffer is None or fake_buffer is None:
            return _learn_n_mb(self, n_steps, real_buffer, fake_buffer, batch_size, real_ratio)      # raises
        real_rows = int(batch_size * real_ratio)
        rows = (real_rows, int(batch_size) - real_rows)
        if rows != self._rows:
            if self._eng is not None:
                carried = self._unbind()
                self._rows = rows
                self._rebind_with(carried, rows[0] + rows[1])
            else:
                self._rows = rows
        return _learn_n_mb(self, n_steps, real_buffer, fake_buffer, batch_size, real_ratio)

"""RCSL policies on the HIP engine.  ``RcslPolicy`` (reference: policy/rcsl/rcsl.py:18-163): pred = MLP([obs | rtg]), MSE on the dataset
action.  ``RcslGaussianPolicy`` (policy/rcsl/rcsl_gauss.py:18-168): z = MLP([obs | rtg]), a ``DiagGaussian`` head with a state-conditioned,
clamped sigma, the Gaussian negative log-likelihood of the dataset action.  Both share everything but the network tail (``_RcslBase``).

The return-to-go travels where the other algorithms carry the reward (``orl_batch.rewards``, the ``rew`` column of a ``DeviceBuffer``).
``learn_epoch`` is the reference trainer's inner loop -- one pass over a shuffled dataset, every row once, last batch partial -- as one
engine call over a caller-supplied row order (``orl_learn_epoch``).  ``rollout()`` (rcsl.py:57-120) rolls a behaviour policy -- here
``AutoregressivePolicy``, or anything with the diffusion policy's interface -- through a dynamics model on the host.
``rollout_device()`` is the same rollout with every array in HBM (``TrajStore``: ``orl_traj_*``); its ``DeviceRollout`` exports the
trajectories above a return threshold straight into the ``DeviceBuffer`` ``learn_epoch`` reads, and ``collect_rollouts_device`` is the
collection loop of run_mbrcsl.py around the two.
"""
from __future__ import annotations

from collections import defaultdict
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from .. import _engine
from .base_policy import EnginePolicy, _adam_hyper, _backbone_dims


def epoch_order(n_rows: int, batch_size: int, n_runs: int = 1, generator: Optional[torch.Generator] = None) -> np.ndarray:
    """Row order of one epoch, int64 [n_runs, ceil(n_rows / B) * B]: one ``torch.randperm(n_rows)`` per run (the index stream of a
    ``DataLoader(shuffle=True)`` sampler, drawn in run order from the global generator unless one is given), padded at the tail with -1."""
    steps = -(-int(n_rows) // int(batch_size))
    order = np.full((int(n_runs), steps * int(batch_size)), -1, dtype=np.int64)
    for r in range(int(n_runs)):
        order[r, :n_rows] = torch.randperm(int(n_rows), generator=generator).numpy()
    return order


class DeviceRollout:
    """What ``rollout_device`` leaves in HBM: a finished ``TrajStore`` (rows with trajectory index, accumulated return, return-to-go)."""

    def __init__(self, store: "_engine.TrajStore", rows: int) -> None:
        self.store = store
        self.rows = int(rows)

    def to_host(self) -> Dict[str, np.ndarray]:
        """the transition dict of ``rollout()``: its keys in its order, its shapes and dtypes"""
        d = self.store.read(0, self.rows)
        return {"obss": d["obs"], "next_obss": d["next_obs"], "actions": d["act"], "rewards": d["rew"][:, None],
                "terminals": d["term"][:, None] != 0.0, "traj_idxs": d["traj_idx"].astype(np.int64), "acc_rets": d["acc_ret"],
                "rtgs": d["rtg"][:, None]}

    def export(self, device_buffer_ring, threshold: Optional[float] = None) -> Tuple[int, int]:
        """Appends the rows of the trajectories with ``returns > threshold`` (every row without a threshold) to the reserved ring
        ``device_buffer_ring``, returns-to-go in its reward column -> (rows kept, trajectories kept)."""
        return self.store.export(device_buffer_ring, threshold)


class _EpochPolicy(EnginePolicy):
    """what the policies trained by ``RcslPolicyTrainer`` share (the two return-conditioned ones and ``AutoregressivePolicy``): a step on
    named batch arrays and ``learn_epoch``"""

    def _step_on(self, batch: Dict, fields) -> Dict[str, float]:
        """One gradient step; ``fields``: (orl_batch slot, batch key, 1 for a per-row scalar that may come without its column axis)"""
        R = self._n_runs
        obs = batch["observations"]
        if np.ndim(obs) not in (2, 3):
            raise ValueError(f"observations: expected [B, obs_dim] or [n_runs, B, obs_dim], got shape {tuple(obs.shape)}")
        B = int(obs.shape[-2])
        self._bind(B)
        dev = self._arena.device
        keep, ptrs = [], {}
        for k, name, cols in fields:
            t = torch.as_tensor(batch[name], dtype=torch.float32, device=dev)
            if cols == 1 and (t.dim() == 1 or (t.dim() == 2 and t.shape[-1] != 1)):
                t = t.unsqueeze(-1)                          # rtgs as [B] / [n_runs, B]
            if t.dim() == 2:
                t = t.unsqueeze(0).expand(R, *t.shape)
            elif t.dim() != 3 or t.shape[0] != R:
                raise ValueError(f"{name}: shape {tuple(t.shape)} is neither [rows, cols] nor [n_runs = {R}, rows, cols]")
            if t.shape[1] != B:
                raise ValueError(f"{name}: {t.shape[1]} rows, observations have {B}")
            t = t.contiguous()
            keep.append(t)
            ptrs[k] = t.data_ptr()
        self._push_lrs()
        torch.cuda.current_stream(dev).synchronize()
        return self._result(self._eng.step(ptrs, None, on_device=True))

    def learn_epoch(self, device_buffer, order, batch_size: int = 256) -> Dict[str, float]:
        """One ordered pass over ``device_buffer`` (rtgs in its reward column): step s of run r learns rows
        ``order[r, s * B : (s + 1) * B]``, negative entries are padding (``epoch_order`` builds such an order).  ``order``: int64
        [n_runs, len] (or [len], shared by the runs) numpy array, or a torch tensor on the engine's device.  Returns the per-key means
        over the steps -- what ``logger.logkv_mean`` per batch holds at the end of the reference's epoch."""
        self._bind(int(batch_size))
        if self._attached is not device_buffer:
            self._eng.attach_buffer(device_buffer)
            self._attached = device_buffer
        self._push_lrs()
        if isinstance(order, torch.Tensor) and order.device.type == "cuda":
            o = order.to(dtype=torch.int64)
            if o.dim() == 1:
                o = o.unsqueeze(0).expand(self._n_runs, -1)
            if o.dim() != 2 or o.shape[0] != self._n_runs:
                raise ValueError(f"order: expected [n_runs = {self._n_runs}, order_len], got {tuple(o.shape)}")
            o = o.contiguous()
            torch.cuda.current_stream(o.device).synchronize()
            m, ms = self._eng.learn_epoch((o.data_ptr(), int(o.shape[1])), on_device=True)
        else:
            m, ms = self._eng.learn_epoch(order.cpu().numpy() if isinstance(order, torch.Tensor) else order)
        self.last_learn_epoch_ms = ms
        return self._result(m)


class _RcslBase(_EpochPolicy):
    """what the two return-conditioned policies share: the constructor, the backbone check, ``learn`` on {observations, actions, rtgs}
    and ``rollout``"""

    def __init__(self, dynamics, rollout_policy, rcsl: nn.Module, rcsl_optim: torch.optim.Optimizer, device="cpu") -> None:
        super().__init__()
        self.dynamics = dynamics
        self.rollout_policy = rollout_policy
        self.rcsl = rcsl
        self.rcsl_optim = rcsl_optim
        self.device = device
        _adam_hyper(rcsl_optim)
        self._dims()

    def _dims(self):
        in_dim, outs = _backbone_dims(self.rcsl.backbone)
        if len(outs) < 2:
            raise NotImplementedError(f"{type(self).__name__} expects MLP(obs_dim + 1, hidden_dims, output_dim=act_dim): at least one hidden layer and the output layer")
        hidden, act_dim = outs[:-1], outs[-1]
        if len(hidden) > _engine.MAX_HIDDEN:
            raise NotImplementedError(f"the HIP engine supports up to {_engine.MAX_HIDDEN} hidden layers, the backbone has {len(hidden)}")
        n_mods = len(list(self.rcsl.backbone.model))
        if n_mods != 2 * len(hidden) + 1 or getattr(self.rcsl.backbone, "activation_cls", nn.ReLU) is not nn.ReLU:
            raise NotImplementedError(f"{type(self).__name__} expects a [Linear, ReLU] x L + Linear backbone")
        return in_dim - 1, act_dim, hidden

    def _nets(self):
        return {_engine.NET_ACTOR: self.rcsl}

    def _optims(self):
        return {_engine.OPT_ACTOR: self.rcsl_optim}

    def _config(self) -> Dict:
        od, ad, hidden = self._dims()
        return dict(obs_dim=od, act_dim=ad, hidden=hidden, actor_lr=float(self.rcsl_optim.param_groups[0]["lr"]))

    def rollout(self, init_obss: np.ndarray, rollout_length: int) -> Tuple[Dict[str, np.ndarray], Dict]:
        """Rolls ``rollout_policy`` through ``dynamics`` from ``init_obss`` for up to ``rollout_length`` steps, a batch of trajectories at a
        time (rcsl.py:57-120).  Transitions: obss, next_obss, actions, rewards [N, 1], terminals [N, 1], traj_idxs [N], acc_rets [N] (the
        return accumulated BEFORE the transition), rtgs [N, 1] = the trajectory's return - acc_rets; info: num_transitions, reward_mean,
        returns [trajectories].  A rollout policy with ``sample_init_noise`` (the diffusion interface) gets its per-trajectory noise,
        thinned to the surviving trajectories, as ``select_action``'s second argument; any other one (``AutoregressivePolicy``) gets None."""
        if self.dynamics is None or self.rollout_policy is None:
            raise NotImplementedError(f"{type(self).__name__}.rollout needs both a dynamics model and a rollout (behaviour) policy; "
                                      f"this policy was built with dynamics={self.dynamics!r}, rollout_policy={self.rollout_policy!r}")
        num_transitions = 0
        rewards_arr = np.array([])
        rollout_transitions = defaultdict(list)
        valid_idxs = np.arange(init_obss.shape[0])      # trajectories still running
        returns = np.zeros(init_obss.shape[0])          # return of every trajectory
        acc_returns = np.zeros(init_obss.shape[0])      # return accumulated so far, of the running ones
        observations = init_obss
        frozen = hasattr(self.rollout_policy, "sample_init_noise")
        frozen_noise = self.rollout_policy.sample_init_noise(init_obss.shape[0]) if frozen else None
        # a dynamics that carries recurrent state per trajectory (RNNDynamics) starts it here and is told every step which trajectories
        # the rows belong to; any other one takes the rows alone
        stateful = bool(getattr(self.dynamics, "stateful", False))
        if stateful:
            self.dynamics.reset_state(init_obss.shape[0])
        for _ in range(rollout_length):
            actions = self.rollout_policy.select_action(observations, frozen_noise)
            if stateful:
                next_observations, rewards, terminals, info = self.dynamics.step_state(observations, actions, valid_idxs)
            else:
                next_observations, rewards, terminals, info = self.dynamics.step(observations, actions)
            rollout_transitions["obss"].append(observations)
            rollout_transitions["next_obss"].append(next_observations)
            rollout_transitions["actions"].append(actions)
            rollout_transitions["rewards"].append(rewards)
            rollout_transitions["terminals"].append(terminals)
            rollout_transitions["traj_idxs"].append(valid_idxs)
            rollout_transitions["acc_rets"].append(acc_returns)
            num_transitions += len(observations)
            rewards_arr = np.append(rewards_arr, rewards.flatten())
            returns[valid_idxs] = returns[valid_idxs] + rewards.flatten()
            acc_returns = acc_returns + rewards.flatten()
            nonterm_mask = (~terminals).flatten()
            if nonterm_mask.sum() == 0:
                break
            observations = next_observations[nonterm_mask]
            valid_idxs = valid_idxs[nonterm_mask]
            acc_returns = acc_returns[nonterm_mask]
            if frozen:
                frozen_noise = frozen_noise[nonterm_mask]
        for k, v in rollout_transitions.items():
            rollout_transitions[k] = np.concatenate(v, axis=0)
        rtgs = returns[rollout_transitions["traj_idxs"]] - rollout_transitions["acc_rets"]
        rollout_transitions["rtgs"] = rtgs[..., None]
        return rollout_transitions, {"num_transitions": num_transitions, "reward_mean": rewards_arr.mean(), "returns": returns}

    def rollout_device(self, init_obss, rollout_length: int, store: Optional["_engine.TrajStore"] = None, fused: bool = False,
                       lag: int = 2) -> Tuple[DeviceRollout, Dict]:
        """``rollout`` with every array on the device: actions from ``rollout_policy.select_action_device``, the model step from
        ``dynamics.step_device``, the bookkeeping in a ``TrajStore`` (termination test, rows, per-trajectory returns, the stable compaction
        of the survivors).  One host read per model step -- the survivor count, which sizes the next step --, then the returns and the
        reward sum.  The compaction keeps the surviving rows in their order, so the policy's ``torch.randn`` draw and the dynamics' Philox
        draws, both keyed by row position, are the ones the host rollout consumes.  A rollout policy with ``device_frozen_noise = True``,
        ``sample_init_noise`` and ``select_action_device(obs, init_noise)`` (``DiffusionBC``) gets its per-trajectory noise [n_traj, 1,
        act_dim], drawn once, and every step the live trajectory indices (``store.live_index()``) as ``noise_index``: the policy's sampler
        gathers the rows.  ``store``: a ``TrajStore`` to reuse (reset here);
        by default a new one of ``len(init_obss) * rollout_length`` rows.  -> (DeviceRollout, info with the keys of ``rollout``)

        ``fused=True`` runs the whole rollout as one device loop (``orl_mbrcsl_rollout``): every launch of every model step is enqueued
        on the policy engine's stream and the host never waits for the step it has just enqueued -- step t is sized by the survivor
        count of step ``t - 1 - lag``, a valid upper bound because survivor counts never increase (``lag = 0``: exact sizes, one wait per
        step).  The normals are ONE ``torch.randn((rollout_length, n_traj, act_dim))`` on the device, step t reading the first rows of
        slice t, so ``torch.manual_seed`` still reproduces a rollout; that draw differs from the per-step ``randn((n, act_dim))`` of
        ``rollout`` and of ``fused=False``, so the results are equal in distribution, not in bits.  The reward is ``raw - penalty_coef *
        penalty`` also at ``penalty_coef = 0``.  ``info`` additionally carries ``steps_enqueued`` and ``loop_ms`` (the HIP-event time of
        the loop).  Not implemented (``NotImplementedError``): a stateful dynamics, a frozen-noise policy, several runs on either side, a
        policy that is not an ``AutoregressivePolicy``."""
        if self.dynamics is None or self.rollout_policy is None:
            raise NotImplementedError(f"{type(self).__name__}.rollout_device needs both a dynamics model and a rollout (behaviour) policy; "
                                      f"this policy was built with dynamics={self.dynamics!r}, rollout_policy={self.rollout_policy!r}")
        dyn, pol = self.dynamics, self.rollout_policy
        if fused:
            return self._rollout_fused(dyn, pol, init_obss, rollout_length, store, lag)
        kind = getattr(dyn, "term_kind", None)
        if kind is None or not hasattr(dyn, "step_device"):
            raise NotImplementedError("rollout_device: the dynamics' termination function is not one of the fixed row-wise tests of "
                                      "utils.termination_fns (an obs_unnormalization wrapper, door or another callable carries no term_kind): "
                                      "the device rollout cannot evaluate it; use rollout()")
        frozen = bool(getattr(pol, "device_frozen_noise", False)) and hasattr(pol, "select_action_device") and hasattr(pol, "sample_init_noise")
        if not frozen and (hasattr(pol, "sample_init_noise") or not hasattr(pol, "select_action_device")):
            raise NotImplementedError(f"rollout_device: the rollout policy {type(pol).__name__} has no select_action_device (a policy with "
                                      "sample_init_noise, the frozen-noise interface, is host-only): use rollout()")
        n_traj, L = int(len(init_obss)), int(rollout_length)
        if n_traj < 1 or L < 1:
            raise ValueError(f"rollout_device: {n_traj} initial states, rollout_length {L}")
        obs = init_obss if isinstance(init_obss, torch.Tensor) else torch.as_tensor(np.asarray(init_obss, dtype=np.float32))
        if obs.device.type != "cuda":
            pdev = torch.device(getattr(pol, "device", "cuda"))
            obs = obs.to(pdev if pdev.type == "cuda" else torch.device("cuda", torch.cuda.current_device()))
        obs = obs.to(torch.float32).reshape(n_traj, -1).contiguous()
        dev = obs.device
        if store is None:
            store = _engine.TrajStore(int(obs.shape[1]), int(pol.act_dim), n_traj, n_traj * L, dev.index or 0)
        store.reset(n_traj)
        # the frozen-noise interface on the device (DiffusionBC): one draw per trajectory; every step the sampler gathers the rows of
        # the live trajectories -- the rows rollout() keeps by thinning its copy
        noise = pol.sample_init_noise(n_traj) if frozen else None
        stateful = bool(getattr(dyn, "stateful", False))      # (as in rollout(): the recurrent state of the trajectories, by index)
        if stateful:
            dyn.reset_state(n_traj)
        with torch.no_grad():
            for _ in range(L):
                if frozen:
                    act = pol.select_action_device(obs, noise, noise_index=store.live_index())
                else:
                    act = pol.select_action_device(obs)
                act = act.to(torch.float32).contiguous()
                nxt, rew, _ = dyn.step_device(obs, act, store.live_index()) if stateful else dyn.step_device(obs, act)
                alive = torch.empty_like(nxt)
                n_alive = store.append_step(kind, obs, act, nxt.contiguous(), rew.contiguous(), alive)
                if n_alive == 0:
                    break
                obs = alive[:n_alive]
        rows, rew_sum, returns = store.finish()
        return DeviceRollout(store, rows), {"num_transitions": rows, "reward_mean": rew_sum / rows, "returns": returns}

    def _rollout_fused(self, dyn, pol, init_obss, rollout_length: int, store, lag: int) -> Tuple[DeviceRollout, Dict]:
        """``rollout_device(fused=True)``"""
        who = "rollout_device(fused=True)"
        kind = getattr(dyn, "term_kind", None)
        if kind is None:
            raise NotImplementedError(f"{who}: the dynamics carries no term_kind (its termination function is not one of the fixed row-wise "
                                      "tests of utils.termination_fns): the device loop cannot evaluate it; use rollout()")
        if bool(getattr(dyn, "stateful", False)):
            raise NotImplementedError(f"{who}: a stateful dynamics ({type(dyn).__name__} carries recurrent state per trajectory) is stepped "
                                      "through the live trajectory indices, which the loop does not hand out; use fused=False")
        if bool(getattr(pol, "device_frozen_noise", False)) or hasattr(pol, "sample_init_noise"):
            raise NotImplementedError(f"{who}: a frozen-noise policy ({type(pol).__name__} has sample_init_noise) gathers its noise by "
                                      "live trajectory index every step; use fused=False")
        for name, obj in (("rollout policy", pol), ("dynamics", dyn)):
            runs = int(getattr(obj, "n_runs", getattr(obj, "_n_runs", 1)))
            if runs != 1:
                raise NotImplementedError(f"{who}: the {name} has n_runs = {runs}; the loop rolls one run through one run")
        if not hasattr(pol, "loop_engine") or not hasattr(dyn, "loop_engine"):
            raise NotImplementedError(f"{who}: needs an AutoregressivePolicy and an EnsembleDynamics (the device loop drives their engines "
                                      f"directly), got {type(pol).__name__} and {type(dyn).__name__}; use fused=False")
        n_traj, L = int(len(init_obss)), int(rollout_length)
        if n_traj < 1 or L < 1:
            raise ValueError(f"rollout_device: {n_traj} initial states, rollout_length {L}")
        if int(lag) < 0:
            raise ValueError(f"rollout_device: lag {lag} must be >= 0")
        peng = pol.loop_engine()
        deng, mode, coef = dyn.loop_engine()
        dev = torch.device("cuda", int(peng.cfg.device))
        obs = init_obss if isinstance(init_obss, torch.Tensor) else torch.as_tensor(np.asarray(init_obss, dtype=np.float32))
        obs = obs.to(device=dev, dtype=torch.float32).reshape(n_traj, -1).contiguous()
        if store is None:
            store = _engine.TrajStore(int(obs.shape[1]), int(pol.act_dim), n_traj, n_traj * L, dev.index or 0)
        eps = torch.randn((L, n_traj, int(pol.act_dim)), device=dev)
        torch.cuda.current_stream(dev).synchronize()
        rows, rew_sum, returns, enq, ms = peng.mbrcsl_rollout(deng, store, obs.data_ptr(), n_traj, L, kind, mode, coef, eps.data_ptr(), int(lag))
        return DeviceRollout(store, rows), {"num_transitions": rows, "reward_mean": rew_sum / rows, "returns": returns,
                                            "steps_enqueued": enq, "loop_ms": ms}

    def learn(self, batch: Dict) -> Dict[str, float]:
        """One gradient step on ``{"observations", "actions", "rtgs"}``: [B, ...] arrays shared by every run or [n_runs, B, ...]."""
        return self._step_on(batch, (("observations", "observations", None), ("actions", "actions", None), ("rewards", "rtgs", 1)))

    def _backbone_runs(self, obs, rtg):
        """-> (backbone output of EVERY run [n_runs, E, act_dim] in one batched forward, the stacked net tensors); ``obs`` [n_runs, E,
        obs_dim], ``rtg`` [n_runs, E] or [n_runs, E, 1]"""
        if self._eng is None:
            raise RuntimeError("select_action_runs before the first learn(): no engine is bound yet")
        P = self._stacked_net(_engine.NET_ACTOR)
        o = torch.as_tensor(np.asarray(obs, dtype=np.float32), device=self._arena.device)
        g = torch.as_tensor(np.asarray(rtg, dtype=np.float32), device=self._arena.device)
        if g.dim() == 2:
            g = g.unsqueeze(-1)
        h = torch.cat([o, g], dim=-1)
        idx = sorted(int(k[len("backbone.model."):-len(".weight")]) for k in P if k.startswith("backbone.model.") and k.endswith(".weight"))
        for n, i in enumerate(idx):
            h = torch.baddbmm(P[f"backbone.model.{i}.bias"].unsqueeze(1), h, P[f"backbone.model.{i}.weight"].transpose(1, 2))
            if n + 1 < len(idx):
                h = torch.relu(h)
        return h, P


class RcslPolicy(_RcslBase):
    ALGO = "rcsl"

    def select_action(self, obs: np.ndarray, rtg) -> np.ndarray:
        with torch.no_grad():
            action = self.rcsl.forward(obs, rtg)
        return action.cpu().numpy()

    def select_action_runs(self, obs: np.ndarray, rtg: np.ndarray) -> np.ndarray:
        """Actions of EVERY run in one batched forward: ``obs`` [n_runs, E, obs_dim], ``rtg`` [n_runs, E] or [n_runs, E, 1]"""
        with torch.no_grad():
            return self._backbone_runs(obs, rtg)[0].cpu().numpy()


class RcslGaussianPolicy(_RcslBase):
    """``rcsl`` is a ``RcslGaussianModule``: an ``MLP(obs_dim + 1, hidden, output_dim=act_dim)`` backbone and
    ``DiagGaussian(act_dim, act_dim, unbounded=True, conditioned_sigma=True)`` with the default clamp (-5, 2) -- what run_rcsl_gauss.py
    builds; anything else is refused.  ``learn`` reads the clamped head output as a log-variance, ``select_action`` samples
    ``Normal(mu, exp(that output))``: the reference's asymmetry, reproduced."""
    ALGO = "rcsl_gauss"
    SIGMA_BOUNDS = (-5.0, 2.0)

    def _dims(self):
        od, act_dim, hidden = super()._dims()
        dist = getattr(self.rcsl, "dist_net", None)
        if dist is None or not hasattr(dist, "mu"):
            raise NotImplementedError("RcslGaussianPolicy expects a RcslGaussianModule(backbone, DiagGaussian)")
        if not getattr(dist, "_unbounded", False):
            raise NotImplementedError("RcslGaussianPolicy: DiagGaussian(unbounded=False) (mu = max_mu * tanh) is not implemented by the HIP engine")
        if not getattr(dist, "_c_sigma", False):
            raise NotImplementedError("RcslGaussianPolicy: DiagGaussian(conditioned_sigma=False) (a free sigma_param) is not implemented by the HIP engine")
        if dist.mu.in_features != act_dim or dist.mu.out_features != act_dim or dist.sigma.in_features != act_dim or dist.sigma.out_features != act_dim:
            raise NotImplementedError(f"RcslGaussianPolicy: DiagGaussian must have latent_dim == output_dim == act_dim = {act_dim} (the backbone's "
                                      f"output), got {dist.mu.in_features} -> {dist.mu.out_features}")
        if (float(dist._sigma_min), float(dist._sigma_max)) != self.SIGMA_BOUNDS:
            raise NotImplementedError(f"RcslGaussianPolicy: the HIP engine clamps the sigma head to {self.SIGMA_BOUNDS} (DiagGaussian's "
                                      f"defaults), got ({dist._sigma_min}, {dist._sigma_max})")
        return od, act_dim, hidden

    def select_action(self, obs: np.ndarray, rtg) -> np.ndarray:
        with torch.no_grad():
            action = self.rcsl.forward(obs, rtg).rsample()
        return action.cpu().numpy()

    def select_action_runs(self, obs: np.ndarray, rtg: np.ndarray, deterministic: bool = False) -> np.ndarray:
        """Actions of EVERY run in one batched forward: ``obs`` [n_runs, E, obs_dim], ``rtg`` [n_runs, E] or [n_runs, E, 1].  Sampled as
        ``select_action`` samples; ``deterministic``: the mean."""
        with torch.no_grad():
            z, P = self._backbone_runs(obs, rtg)
            mu = torch.baddbmm(P["dist_net.mu.bias"].unsqueeze(1), z, P["dist_net.mu.weight"].transpose(1, 2))
            if deterministic:
                return mu.cpu().numpy()
            s = torch.baddbmm(P["dist_net.sigma.bias"].unsqueeze(1), z, P["dist_net.sigma.weight"].transpose(1, 2)).clamp(*self.SIGMA_BOUNDS)
            return (mu + s.exp() * torch.randn_like(mu)).cpu().numpy()


def collect_rollouts_device(policy, init_obss_dataset, rollout_batch: int, horizon: int, threshold: float, num_need_traj: int, max_epochs: int,
                            capacity_rows: int, rng=np.random, fused: bool = False):
    """The collection loop of run_mbrcsl.py (``get_rollout_trajs``) on the device: per epoch ``rollout_batch`` initial states drawn with
    ``rng.randint`` from ``init_obss_dataset`` [M, obs_dim], one ``policy.rollout_device`` of up to ``horizon`` steps, and the export of
    the trajectories with ``returns > threshold`` into ONE ring of ``capacity_rows`` rows; until ``num_need_traj`` trajectories have been
    kept or ``max_epochs`` epochs have run.  ``fused``: passed to ``rollout_device``.  -> (the ring: a ``DeviceBuffer`` with returns-to-go in its reward column, ready for
    ``learn_epoch``; info: num_traj, returns (of the kept trajectories, float64), max_return (their maximum, -inf when none was
    kept), epochs)"""
    if int(max_epochs) < 1 or int(rollout_batch) < 1 or int(num_need_traj) < 1:
        raise ValueError(f"collect_rollouts_device: max_epochs {max_epochs}, rollout_batch {rollout_batch}, num_need_traj {num_need_traj}: "
                         "each must be at least 1")
    init = np.asarray(init_obss_dataset, dtype=np.float32)
    init = init.reshape(len(init), -1)
    ring, store = None, None
    kept, num_traj, epochs = [], 0, 0
    while num_traj < int(num_need_traj) and epochs < int(max_epochs):
        idx = rng.randint(len(init), size=int(rollout_batch))
        roll, info = policy.rollout_device(init[idx], horizon, store=store, **({"fused": True} if fused else {}))
        if store is None:                      # (the first rollout made the store; every later one reuses it)
            store = roll.store
            ring = _engine.DeviceBuffer(store.obs_dim, store.act_dim, store.device)
            ring.reserve(int(capacity_rows))
        _, n_kept = roll.export(ring, threshold)
        returns = info["returns"]
        kept.append(returns[returns > threshold])
        num_traj += n_kept
        epochs += 1
    returns = np.concatenate(kept)
    return ring, {"num_traj": num_traj, "returns": returns, "max_return": float(returns.max()) if len(returns) else -np.inf, "epochs": epochs}

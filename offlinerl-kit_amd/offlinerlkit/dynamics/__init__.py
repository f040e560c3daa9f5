"""The dynamics ensemble of the model-based algorithms (reference: dynamics/base_dynamics.py, dynamics/ensemble_dynamics.py) on the HIP
engine (``orl_dyn_*`` of include/orl_engine.h, csrc/dynamics.hip).

``EnsembleDynamics`` keeps the reference's host logic -- the holdout split, the scaler, the bootstrap and shuffle indices, the 1 %
improvement rule, the elites, the logger keys, ``save`` / ``load`` -- and consumes the host RNGs in the reference's order
(``torch.utils.data.random_split``, ``np.random.randint``, ``np.random.uniform`` per epoch).  The arithmetic runs on the device: one
``learn()`` epoch is one call that enqueues every minibatch without a host round trip, ``validate`` and ``step`` are one call each.

``step`` draws its Gaussian noise and its elite per row from a device Philox stream by default (``seed`` of
``set_engine_options``): the reference's ``np.random.normal`` / ``np.random.choice`` stream cannot be reproduced on the device, so
the samples are distributed like the reference's, not equal to them.  Pass ``noise`` / ``model_idxs`` to ``step`` to teacher-force
the reference's draws.

Multi-run: ``set_engine_options(n_runs=R)`` trains R independent ensembles (runs) in the same launches.  Each run has its own holdout
split, scaler, bootstrap indices, early-stopping counter and elites; ``train`` loops until every run has stopped.  The torch module
shows the run chosen by ``select_run`` (run 0 by default).

RAMBO's adversarial update (``bind_adversary``, ``adv_forward`` / ``adv_update`` and their ``_device`` forms; ``orl_dynadv_*``) trains
the same parameters with a second optimizer whose Adam state is separate from ``optim``'s; ``save`` / ``load`` are unchanged.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from .. import _engine
from ..utils.scaler import StandardScaler


class BaseDynamics(object):
    def __init__(self, model: nn.Module, optim: torch.optim.Optimizer) -> None:
        super().__init__()
        self.model = model
        self.optim = optim

    def step(self, obs: np.ndarray, action: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, Dict]:
        raise NotImplementedError

    # ---- what the engine-backed models share.  They keep ``_eng`` (the engine object), ``_arena`` (the torch tensor its parameter
    # blocks live in), ``_shape`` (what the engine was built for) and ``scaler``, and provide ``_drain()``: wait for the engine's
    # work on the arena ----
    def _device(self) -> torch.device:
        dev = self.model.device
        if dev.type != "cuda":
            if not torch.cuda.is_available():
                raise RuntimeError("the dynamics ensemble runs on the HIP engine: no HIP device (MI355X) visible")
            dev = torch.device("cuda", 0)
        return torch.device("cuda", dev.index or 0)

    def _alias_params(self, base: int, tensors) -> None:
        """point the module's parameters at the block ``base`` floats into the arena, laid out by ``tensors``"""
        params = dict(self.model.named_parameters())
        for name, off, shape in tensors:
            params[name].data = self._arena[base + off: base + off + int(np.prod(shape))].view(shape)

    def _unbind(self) -> None:
        if self._eng is None:
            return
        self._drain()
        for p in self.model.parameters():
            p.data = p.data.clone()
        self._eng.close()
        self._eng, self._arena, self._shape = None, None, None

    def save(self, save_path: str) -> None:
        if self._eng is not None:
            self._drain()
        sd = self.model.state_dict()
        torch.save(type(sd)((k, v.detach().clone()) for k, v in sd.items()), os.path.join(save_path, "dynamics.pth"))
        self.scaler.save_scaler(save_path)


def _fresh_model_params(model, seed: int) -> Dict[str, torch.Tensor]:
    """the constructor's initialisation under torch seed ``seed`` (runs r > 0 of a multi-run ensemble)"""
    from ..modules import EnsembleDynamicsModel
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = EnsembleDynamicsModel(model.obs_dim, model.action_dim, model.hidden_dims, model.num_ensemble, model.num_elites,
                                  weight_decays=model.weight_decays, with_reward=bool(model._with_reward))
    return dict(m.named_parameters())


class EnsembleDynamics(BaseDynamics):
    def __init__(self, model: nn.Module, optim: torch.optim.Optimizer, scaler: StandardScaler,
                 terminal_fn: Callable[[np.ndarray, np.ndarray, np.ndarray], np.ndarray], penalty_coef: float = 0.0,
                 uncertainty_mode: str = "aleatoric") -> None:
        super().__init__(model, optim)
        if uncertainty_mode not in _engine.DYN_PENALTY:
            raise ValueError(f"unknown uncertainty_mode {uncertainty_mode!r}")
        self.scaler = scaler
        self.terminal_fn = terminal_fn
        self._penalty_coef = penalty_coef
        self._uncertainty_mode = uncertainty_mode
        self._n_runs, self._seed = 1, 0
        self._eng: Optional[_engine.Dynamics] = None
        self._arena = None
        self._shape = None             # (batch_size, logvar_loss_coef) the engine was built for
        self._cur_run = 0
        self.scalers: List[StandardScaler] = [scaler]
        self._data_key = None
        self._adv_key = None           # (lr, betas, eps, adv_weight, rollout rows, dataset rows) of the bound adversarial optimizer

    # ---- engine binding ----
    def set_engine_options(self, n_runs: int = 1, seed: Optional[int] = None) -> None:
        if self._eng is not None:
            raise RuntimeError("set_engine_options before the first train() / step()")
        self._n_runs = int(n_runs)
        self._seed = int(seed) if seed is not None else 0
        self.scalers = [self.scaler] + [StandardScaler(self.scaler.mu, self.scaler.std) for _ in range(self._n_runs - 1)]

    def _bind(self, batch_size: int = 256, logvar_loss_coef: float = 0.01) -> None:
        shape = (int(batch_size), float(logvar_loss_coef))
        if self._eng is not None and self._shape == shape:
            return
        carried = None
        if self._eng is not None:
            carried = [(self._eng.get_params(r), self._eng.adam_state(r), self._eng.get_elites(r),
                        self._eng.adv_adam_state(r) if self._adv_key is not None else None) for r in range(self._n_runs)]
            self._unbind()
        dev = self._device()
        m = self.model
        g = self.optim.param_groups[0] if self.optim is not None else {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8}
        if self.optim is not None and g.get("weight_decay", 0.0):
            raise NotImplementedError("the dynamics optimizer's own weight_decay is not supported (the model's weight_decays are)")
        cfg = _engine.default_dyn_config(obs_dim=m.obs_dim, act_dim=m.action_dim, hidden=m.hidden_dims, num_ensemble=m.num_ensemble,
                                         num_elites=m.num_elites, with_reward=int(bool(m._with_reward)), weight_decay=m.weight_decays,
                                         lr=float(g["lr"]), adam_beta1=float(g["betas"][0]), adam_beta2=float(g["betas"][1]),
                                         adam_eps=float(g["eps"]), batch_size=shape[0], logvar_loss_coef=shape[1],
                                         n_runs=self._n_runs, device=dev.index, precision=0, seed=self._seed)
        P = int(_engine.load_library().orl_dyn_config_floats(cfg))
        self._arena = torch.zeros(self._n_runs * P, dtype=torch.float32, device=dev)
        cfg.external_arena = self._arena.data_ptr()
        torch.cuda.synchronize(dev)
        self._eng = _engine.Dynamics(cfg)
        self._shape = shape
        m.to(dev)
        m.device = dev
        if self._adv_key is not None:      # the adversarial optimizer follows the parameters into the new engine
            self._adv_configure(self._adv_key)
        for r in range(self._n_runs):
            if carried is not None:
                params, (am, av, t), el, adv = carried[r]
                self._eng.set_params(r, params)
                self._eng.set_adam_state(r, am, av, t)
                self._eng.set_elites(r, el)
                if adv is not None:
                    self._eng.set_adv_adam_state(r, *adv)
                continue
            src = dict(m.named_parameters()) if r == 0 else _fresh_model_params(m, self._seed + r)
            self._eng.set_params(r, {k: v.detach().cpu().numpy() for k, v in src.items() if k != "elites"})
            self._eng.set_elites(r, src["elites"].detach().cpu().numpy())
        self._cur_run = -1
        self.select_run(0)
        self._data_key = None

    def _drain(self) -> None:
        self._eng.sync()

    def select_run(self, run: int) -> None:
        """point the torch module (forward, state_dict, save) and ``self.scaler`` at run ``run``"""
        if self._eng is None:
            if run != 0:
                raise RuntimeError("select_run before the engine exists: only run 0")
            return
        if run == self._cur_run:
            return
        self._alias_params((self._eng.ptr(run) - self._arena.data_ptr()) // 4, self._eng.tensors)
        self.model.set_elites([int(i) for i in self._eng.get_elites(run)])
        self.scaler = self.scalers[run]
        self._cur_run = run

    def _sync_torch(self) -> None:
        torch.cuda.synchronize(self._arena.device)

    def _push_elites_from_model(self) -> None:
        self._eng.set_elites(self._cur_run, self.model.elites.detach().cpu().numpy())

    # ---- reference API ----
    @torch.no_grad()
    def step(self, obs: np.ndarray, action: np.ndarray, noise: Optional[np.ndarray] = None,
             model_idxs: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, Dict]:
        """ensemble_dynamics.py:29-80.  obs (N, obs_dim) for the selected run, or (R, N, obs_dim) for every run.  ``noise``
        (K, N, obs_dim + 1) / (R, K, N, obs_dim + 1) and ``model_idxs`` (N,) / (R, N) teacher-force the reference's draws; by default
        they come from the device Philox stream."""
        self._bind(*(self._shape or (256, 0.01)))
        self._sync_torch()
        self._push_elites_from_model()
        obs = np.asarray(obs, dtype=np.float32)
        action = np.asarray(action, dtype=np.float32)
        batched = obs.ndim == 3
        R = self._n_runs
        if batched:
            o, a, nz, mi = obs, action, noise, model_idxs
        else:
            o, a = np.broadcast_to(obs, (R,) + obs.shape), np.broadcast_to(action, (R,) + action.shape)
            nz = None if noise is None else np.broadcast_to(noise, (R,) + np.shape(noise))
            mi = None if model_idxs is None else np.broadcast_to(model_idxs, (R,) + np.shape(model_idxs))
        for r in range(R):
            sc = self.scalers[r]
            if sc.mu is None:
                raise RuntimeError("the scaler is not fitted: train() or load() the dynamics first")
            self._eng.set_scaler(r, sc.mu, sc.std)
        nxt, rew, raw, pen, midx = self._eng.step(o, a, nz, mi, self._uncertainty_mode, float(self._penalty_coef))
        if not batched:
            r = self._cur_run
            nxt, rew, raw, pen, midx = nxt[r], rew[r], raw[r], pen[r], midx[r]
        reward = rew[..., None]
        terminal = self.terminal_fn(obs, action, nxt)
        info = {"raw_reward": raw[..., None], "model_idxs": midx}
        if self._penalty_coef:
            info["penalty"] = pen[..., None]
        return nxt, reward if self._penalty_coef else raw[..., None], terminal, info

    @property
    def term_kind(self) -> Optional[int]:
        """the ``TERM_*`` kind of the termination function (utils.termination_fns), None when it is not a fixed row-wise test"""
        from ..utils import termination_fns
        return termination_fns.term_kind(self.terminal_fn)

    @torch.no_grad()
    def step_device(self, obs: torch.Tensor, action: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, Dict]:
        """``step`` without the termination function, on tensors of the engine's device and without a host round trip: obs (N, obs_dim),
        action (N, act_dim) -> (next_obs (N, obs_dim), reward (N,), info).  Same scaler, elites and penalty handling as ``step``; the
        draws come from the device Philox stream (the same stream, keyed by the call counter, as ``step`` without teacher forcing).
        With several runs every run steps the same rows and the selected run's outputs are returned.  The termination test is left to
        the consumer (``DeviceBuffer.append_rollout`` runs ``term_kind`` on the device)."""
        self._bind(*(self._shape or (256, 0.01)))
        self._sync_torch()
        self._push_elites_from_model()
        dev = self._arena.device
        R = self._n_runs
        o = torch.as_tensor(obs, dtype=torch.float32, device=dev)
        a = torch.as_tensor(action, dtype=torch.float32, device=dev)
        if o.dim() != 2 or a.dim() != 2 or o.shape[0] != a.shape[0]:
            raise ValueError(f"step_device: obs {tuple(o.shape)} / action {tuple(a.shape)} must be (N, obs_dim) / (N, act_dim)")
        for r in range(R):
            sc = self.scalers[r]
            if sc.mu is None:
                raise RuntimeError("the scaler is not fitted: train() or load() the dynamics first")
            self._eng.set_scaler(r, sc.mu, sc.std)
        nxt, rew, raw, pen = self._eng.step_device(o.unsqueeze(0).expand(R, *o.shape).contiguous(), a.unsqueeze(0).expand(R, *a.shape).contiguous(),
                                                   self._uncertainty_mode, float(self._penalty_coef))
        r = self._cur_run
        info = {"raw_reward": raw[r]}
        if self._penalty_coef:
            info["penalty"] = pen[r]
        return nxt[r], (rew[r] if self._penalty_coef else raw[r]), info

    def loop_engine(self):
        """What a device loop steps through (``RcslPolicy.rollout_device(fused=True)``): the engine after what ``step_device`` does
        before every step -- bind, elites, scaler --, once.  -> (engine, penalty mode code, penalty coefficient)"""
        self._bind(*(self._shape or (256, 0.01)))
        self._sync_torch()
        self._push_elites_from_model()
        for r in range(self._n_runs):
            sc = self.scalers[r]
            if sc.mu is None:
                raise RuntimeError("the scaler is not fitted: train() or load() the dynamics first")
            self._eng.set_scaler(r, sc.mu, sc.std)
        return self._eng, _engine.DYN_PENALTY[self._uncertainty_mode], float(self._penalty_coef)

    @torch.no_grad()
    def step_device_runs(self, obs: torch.Tensor, action: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, Dict]:
        """``step_device`` for R row blocks at once: obs (R, N, obs_dim), action (R, N, act_dim) -> (next_obs (R, N, obs_dim), reward
        (R, N), info).  With ``n_runs == R`` ensembles block r is stepped by run r; with ONE ensemble the blocks are folded into that
        run's rows (R * N rows of one call, so block r's Philox draws are keyed by the row positions r * N ...).  Any other number of
        runs is refused.  Rows that are padding must hold finite values; their outputs mean nothing."""
        self._bind(*(self._shape or (256, 0.01)))
        self._sync_torch()
        self._push_elites_from_model()
        dev = self._arena.device
        o = torch.as_tensor(obs, dtype=torch.float32, device=dev)
        a = torch.as_tensor(action, dtype=torch.float32, device=dev)
        if o.dim() != 3 or a.dim() != 3 or o.shape[:2] != a.shape[:2]:
            raise ValueError(f"step_device_runs: obs {tuple(o.shape)} / action {tuple(a.shape)} must be (R, N, obs_dim) / (R, N, act_dim)")
        R, n = int(o.shape[0]), int(o.shape[1])
        if self._n_runs not in (1, R):
            raise ValueError(f"step_device_runs: {R} row blocks need a dynamics of {R} runs or of one (shared) run, this one has {self._n_runs}")
        for r in range(self._n_runs):
            sc = self.scalers[r]
            if sc.mu is None:
                raise RuntimeError("the scaler is not fitted: train() or load() the dynamics first")
            self._eng.set_scaler(r, sc.mu, sc.std)
        shared = self._n_runs != R
        o, a = o.contiguous(), a.contiguous()
        if shared:
            o, a = o.view(1, R * n, -1), a.view(1, R * n, -1)
        nxt, rew, raw, pen = self._eng.step_device(o, a, self._uncertainty_mode, float(self._penalty_coef))
        if shared:
            nxt, rew, raw, pen = nxt.view(R, n, -1), rew.view(R, n), raw.view(R, n), pen.view(R, n)
        info = {"raw_reward": raw}
        if self._penalty_coef:
            info["penalty"] = pen
        return nxt, (rew if self._penalty_coef else raw), info

    # ---- RAMBO's adversarial update (rambo.py:129-207; orl_dynadv_* of the engine) ----
    def _adv_configure(self, key) -> None:
        lr, betas, eps, w, ba, bs = key
        self._eng.adv_configure(lr, betas, eps, w, ba, bs)

    def bind_adversary(self, optim: torch.optim.Optimizer, adv_weight: float, rollout_rows: int, sl_rows: int) -> None:
        """bind ``dynamics_adv_optim`` (read for lr / betas / eps; its Adam state lives in the engine, separate from ``optim``'s), the
        weight of the adversarial term and the row counts of a call.  Cheap when nothing changed; a changed row count re-sizes the
        workspaces and keeps the optimizer state."""
        self._bind(*(self._shape or (256, 0.01)))
        if not isinstance(optim, torch.optim.Adam):
            raise NotImplementedError("the adversarial dynamics optimizer must be torch.optim.Adam")
        g = optim.param_groups[0]
        if g.get("weight_decay", 0.0) or g.get("amsgrad", False):
            raise NotImplementedError("Adam weight_decay / amsgrad of the adversarial dynamics optimizer are not supported")
        key = (float(g["lr"]), (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"]), float(adv_weight), int(rollout_rows),
               int(sl_rows))
        if key != self._adv_key:
            self._adv_configure(key)
            self._adv_key = key

    def _adv_ready(self) -> None:
        if self._adv_key is None:
            raise RuntimeError("bind_adversary(optim, adv_weight, rollout_rows, sl_rows) before the adversarial calls")
        self._sync_torch()
        self._push_elites_from_model()
        for r in range(self._n_runs):
            sc = self.scalers[r]
            if sc.mu is None:
                raise RuntimeError("the scaler is not fitted: train() or load() the dynamics first")
            self._eng.set_scaler(r, sc.mu, sc.std)

    def _adv_metrics(self, m: np.ndarray) -> Dict[str, float]:
        return {k: float(v) for k, v in zip(_engine.ADV_METRICS, m[self._cur_run])}

    @torch.no_grad()
    def adv_forward(self, obs, act, sl_obs, sl_act, sl_next_obs, sl_rew, noise: Optional[np.ndarray] = None,
                    model_idxs: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """first half of ``dynamics_step_and_forward`` on numpy arrays: (Ba, obs_dim) rollout rows and (Bs, ..) dataset rows (every
        run sees them) -> (next_obs, reward (Ba,), model_idxs) of the selected run; the sample stays on the device for ``adv_update``.
        ``noise`` (K, Ba, obs_dim + 1) / ``model_idxs`` (Ba,) teacher-force the draws."""
        self._adv_ready()
        R = self._n_runs
        bc = lambda a: None if a is None else np.broadcast_to(np.asarray(a), (R,) + np.shape(a))
        sl_rew = np.asarray(sl_rew, np.float32).reshape(-1)
        nxt, rew, mi = self._eng.adv_forward(bc(obs), bc(act), bc(sl_obs), bc(sl_act), bc(sl_next_obs), bc(sl_rew), bc(noise), bc(model_idxs))
        r = self._cur_run
        return nxt[r], rew[r], mi[r]

    @torch.no_grad()
    def adv_update(self, advantage, active=None) -> Dict[str, float]:
        """second half on a numpy advantage (Ba,), already normalised: the adversarial Adam step; returns ``all_loss``, ``sl_loss``,
        ``adv_loss`` (unweighted) and ``adv_log_prob`` of the selected run"""
        a = np.asarray(advantage, np.float32).reshape(-1)
        return self._adv_metrics(self._eng.adv_update(np.broadcast_to(a, (self._n_runs,) + a.shape), active))

    @torch.no_grad()
    def adv_forward_device(self, obs, act, sl_obs, sl_act, sl_next_obs, sl_rew) -> Tuple[torch.Tensor, torch.Tensor]:
        """``adv_forward`` on tensors (moved to the engine's device if they are elsewhere), draws from the device Philox stream; returns
        device tensors (next_obs (Ba, obs_dim), reward (Ba,))"""
        self._adv_ready()
        dev, R = self._arena.device, self._n_runs

        def prep(x, cols):
            t = torch.as_tensor(x, dtype=torch.float32, device=dev).reshape(-1, cols) if cols else \
                torch.as_tensor(x, dtype=torch.float32, device=dev).reshape(-1)
            return t.unsqueeze(0).expand(R, *t.shape).contiguous()
        od, ad = self.model.obs_dim, self.model.action_dim
        nxt, rew = self._eng.adv_forward_device(prep(obs, od), prep(act, ad), prep(sl_obs, od), prep(sl_act, ad), prep(sl_next_obs, od),
                                                prep(sl_rew, 0))
        return nxt[self._cur_run], rew[self._cur_run]

    @torch.no_grad()
    def adv_update_device(self, advantage: torch.Tensor, active=None) -> Dict[str, float]:
        a = torch.as_tensor(advantage, dtype=torch.float32, device=self._arena.device).reshape(-1)
        return self._adv_metrics(self._eng.adv_update_device(a.unsqueeze(0).expand(self._n_runs, -1).contiguous(), active))

    @torch.no_grad()
    def sample_next_obss_device(self, obs, action, num_samples: int, noise=None) -> torch.Tensor:
        """ensemble_dynamics.py:82-99 on the device (``orl_dynsample_next``): obs (B, obs_dim), action (B, act_dim), tensors or numpy
        arrays -> (num_samples, E, B, obs_dim) on the engine's device, one sample of every ELITE (in ``model.elites`` order) per draw;
        nothing visits the host when the inputs are device tensors.  ``noise`` (num_samples, E, B, obs_dim + 1) teacher-forces the
        reference's ``randn_like`` draws (the reward column is drawn and dropped); by default they come from a device Philox stream
        of this call alone, so ``step``'s draws are what they are without it.  With several runs every run samples the same rows
        and the selected run's samples are returned."""
        self._bind(*(self._shape or (256, 0.01)))
        self._sync_torch()
        self._push_elites_from_model()
        dev, R = self._arena.device, self._n_runs
        o = torch.as_tensor(obs, dtype=torch.float32, device=dev)
        a = torch.as_tensor(action, dtype=torch.float32, device=dev)
        if o.dim() != 2 or a.dim() != 2 or o.shape[0] != a.shape[0]:
            raise ValueError(f"sample_next_obss: obs {tuple(o.shape)} / action {tuple(a.shape)} must be (B, obs_dim) / (B, act_dim)")
        for r in range(R):
            sc = self.scalers[r]
            if sc.mu is None:
                raise RuntimeError("the scaler is not fitted: train() or load() the dynamics first")
            self._eng.set_scaler(r, sc.mu, sc.std)
        nz = None
        if noise is not None:
            nz = torch.as_tensor(noise, dtype=torch.float32, device=dev)
            nz = nz.unsqueeze(0).expand(R, *nz.shape).contiguous()
        out = self._eng.sample_next_device(o.unsqueeze(0).expand(R, *o.shape).contiguous(), a.unsqueeze(0).expand(R, *a.shape).contiguous(),
                                           int(num_samples), nz)
        return out[self._cur_run]

    def sample_next_obss(self, obs, action, num_samples: int) -> torch.Tensor:
        """ensemble_dynamics.py:82-99: (num_samples, E, B, obs_dim) next observations on the dynamics' device (MOBILE's compute_lcb)"""
        return self.sample_next_obss_device(obs, action, num_samples)

    def format_samples_for_training(self, data: Dict) -> Tuple[np.ndarray, np.ndarray]:
        obss = data["observations"]
        actions = data["actions"]
        next_obss = data["next_observations"]
        rewards = data["rewards"]
        delta_obss = next_obss - obss
        inputs = np.concatenate((obss, actions), axis=-1)
        targets = np.concatenate((delta_obss, rewards), axis=-1)
        return inputs, targets

    def _load(self, inputs: np.ndarray, targets: np.ndarray, key) -> None:
        if self._data_key is not key:
            self._eng.load_data(inputs, targets)
            self._data_key = key

    def train(self, data: Dict, logger, max_epochs: Optional[float] = None, max_epochs_since_update: int = 5, batch_size: int = 256,
              holdout_ratio: float = 0.2, logvar_loss_coef: float = 0.01) -> None:
        """ensemble_dynamics.py:111-176 with the arithmetic on the device; returns nothing, like the reference"""
        self._bind(batch_size, logvar_loss_coef)
        self._sync_torch()
        inputs, targets = self.format_samples_for_training(data)
        inputs, targets = np.asarray(inputs, np.float32), np.asarray(targets, np.float32)
        trace = self.train_trace = {"train_idx": [], "holdout_idx": [], "data_idxes": [], "train_loss": [], "holdout_loss": []}
        R, K = self._n_runs, self.model.num_ensemble
        data_size = inputs.shape[0]
        holdout_size = min(int(data_size * holdout_ratio), 1000)
        train_size = data_size - holdout_size
        train_idx, hold_idx, data_idxes = [], [], []
        for r in range(R):
            tr, ho = torch.utils.data.random_split(range(data_size), (train_size, holdout_size))
            tr, ho = np.asarray(tr.indices, np.int64), np.asarray(ho.indices, np.int64)
            self.scalers[r].fit(inputs[tr])
            train_idx.append(tr); hold_idx.append(ho)
            data_idxes.append(np.random.randint(train_size, size=[K, train_size]))
        self.scaler = self.scalers[self._cur_run]
        trace["train_idx"], trace["holdout_idx"] = train_idx, hold_idx
        self._eng.load_data(inputs, targets)
        self._data_key = None
        for r in range(R):
            self._eng.set_scaler(r, self.scalers[r].mu, self.scalers[r].std)
        hold = np.stack(hold_idx)
        holdout_losses = [[1e10] * K for _ in range(R)]
        cnt = [0] * R
        active = np.ones(R, np.int32)
        epoch = 0
        logger.log("Training dynamics:")
        while active.any():
            epoch += 1
            trace["data_idxes"].append([d.copy() for d in data_idxes])
            rows = np.stack([train_idx[r][data_idxes[r]] for r in range(R)])
            train_loss = self._eng.learn_epoch(rows, active)
            new_losses = self._eng.validate(hold)
            trace["train_loss"].append(train_loss.copy()); trace["holdout_loss"].append(new_losses.copy())
            r0 = self._cur_run
            if active[r0]:
                logger.logkv("loss/dynamics_train_loss", float(train_loss[r0]))
                logger.logkv("loss/dynamics_holdout_loss", float(np.sort(new_losses[r0])[:self.model.num_elites].mean()))
                logger.set_timestep(epoch)
                logger.dumpkvs(exclude=["policy_training_progress"])
            for r in range(R):
                if not active[r]:
                    continue
                idxes = np.argsort(np.random.uniform(size=data_idxes[r].shape), axis=-1)
                data_idxes[r] = data_idxes[r][np.arange(K)[:, None], idxes]
                indexes = []
                for i in range(K):
                    new_loss, old_loss = float(new_losses[r][i]), holdout_losses[r][i]
                    if (old_loss - new_loss) / old_loss > 0.01:
                        indexes.append(i)
                        holdout_losses[r][i] = new_loss
                if indexes:
                    mask = np.zeros(K, np.int32)
                    mask[indexes] = 1
                    self._eng.update_save(r, mask)
                    cnt[r] = 0
                else:
                    cnt[r] += 1
                if cnt[r] >= max_epochs_since_update or (max_epochs and epoch >= max_epochs):
                    active[r] = 0
                    trace.setdefault("stop_epoch", [0] * R)[r] = epoch
        self._eng.sync()
        trace["elites"] = []
        for r in range(R):
            el = self.select_elites(holdout_losses[r])
            self._eng.set_elites(r, el)
            self._eng.load_save(r)
            trace["elites"].append(el)
        self._eng.sync()
        cur, self._cur_run = self._cur_run, -1
        self.select_run(cur)
        self.save(logger.model_dir)
        self.model.eval()
        logger.log("elites:{} , holdout loss: {}".format(trace["elites"][cur], (np.sort(holdout_losses[cur])[:self.model.num_elites]).mean()))

    def learn(self, inputs: np.ndarray, targets: np.ndarray, batch_size: int = 256, logvar_loss_coef: float = 0.01) -> float:
        """ensemble_dynamics.py:178-209 on already-scaled [K, n, ...] arrays (every run learns them); returns the selected run's loss"""
        self._bind(batch_size, logvar_loss_coef)
        self._sync_torch()
        K, n = inputs.shape[0], inputs.shape[1]
        self._eng.load_data(np.asarray(inputs, np.float32).reshape(K * n, -1), np.asarray(targets, np.float32).reshape(K * n, -1))
        self._data_key = None
        for r in range(self._n_runs):
            self._eng.set_scaler(r, np.zeros(inputs.shape[-1], np.float32), np.ones(inputs.shape[-1], np.float32))
        rows = np.broadcast_to((np.arange(K)[:, None] * n + np.arange(n)[None, :])[None], (self._n_runs, K, n))
        return float(self._eng.learn_epoch(rows)[self._cur_run])

    @torch.no_grad()
    def validate(self, inputs: np.ndarray, targets: np.ndarray) -> List[float]:
        """ensemble_dynamics.py:211-217 on already-scaled (n, ...) arrays; the selected run's per-member MSE"""
        self._bind(*(self._shape or (256, 0.01)))
        self._sync_torch()
        n = inputs.shape[0]
        self._eng.load_data(np.asarray(inputs, np.float32), np.asarray(targets, np.float32))
        self._data_key = None
        for r in range(self._n_runs):
            self._eng.set_scaler(r, np.zeros(inputs.shape[-1], np.float32), np.ones(inputs.shape[-1], np.float32))
        out = self._eng.validate(np.broadcast_to(np.arange(n)[None], (self._n_runs, n)))
        return list(out[self._cur_run])

    def select_elites(self, metrics: List) -> List[int]:
        pairs = [(metric, index) for metric, index in zip(metrics, range(len(metrics)))]
        pairs = sorted(pairs, key=lambda x: x[0])
        return [pairs[i][1] for i in range(self.model.num_elites)]

    def load(self, load_path: str) -> None:
        if self._eng is not None:
            self._sync_torch()
        state = torch.load(os.path.join(load_path, "dynamics.pth"), map_location=self.model.device)
        if "elites" in state and tuple(state["elites"].shape) != tuple(self.model.elites.shape):
            self.model.set_elites([int(i) for i in state["elites"]])
        self.model.load_state_dict(state)
        self.scaler.load_scaler(load_path)
        self.scalers[self._cur_run] = self.scaler
        if self._eng is not None:
            torch.cuda.synchronize(self._arena.device)
            self._push_elites_from_model()


def rnn_epoch_order(n: int, generator: Optional[torch.Generator] = None) -> np.ndarray:
    """The row order of one epoch of ``DataLoader(data, shuffle=True)`` over ``n`` items, consuming the host torch RNG (``generator``,
    or the global one) exactly as the loader does: its iterator draws a base seed, its ``RandomSampler`` draws the seed of a fresh
    generator, and that generator's ``randperm(n)`` is the order."""
    torch.empty((), dtype=torch.int64).random_(generator=generator)
    seed = int(torch.empty((), dtype=torch.int64).random_(generator=generator).item())
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randperm(n, generator=g).numpy().astype(np.int64)


def _fresh_rnn_params(model, seed: int) -> Dict[str, torch.Tensor]:
    """the constructor's initialisation of ``RNNModel`` under torch seed ``seed`` (runs r > 0 of a multi-run ``RNNDynamics``)"""
    from ..nets import RNNModel
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = RNNModel(model.input_dim, model.output_dim, model.hidden_dims, model.rnn_num_layers, model.dropout_rate)
    return dict(m.state_dict())


class RNNDynamics(BaseDynamics):
    """The GRU sequence dynamics model (reference: dynamics/rnn_dynamics.py over nets/rnn.py:RNNModel) on the HIP engine (``orl_rnn_*``,
    csrc/rnn_dynamics.hip).  ``learn`` is one device step of the masked MSE with Adam, ``train`` loads the data set into HBM once and
    runs every epoch as one call, ``step`` is one eval-mode forward over the windows.  A rollout goes through the carried state
    instead: ``reset_state`` once, then ``step_state`` (numpy) or ``step_device`` (tensors) per model step, O(1) work each at any
    horizon (``RcslPolicy.rollout`` / ``rollout_device`` do this for a ``stateful`` dynamics); ``MBPolicyTrainer``'s MOPO / COMBO
    rollouts and training through the carried state are not supported.  The module's parameters alias the engine's
    block, so ``model.state_dict()``, ``save`` and ``load`` see what the engine trains.  Dropout masks come from a device Philox
    stream, so a training run is distributed like the reference's, not equal to it (at ``dropout_rate`` 0 it is equal).

    Multi-run: ``set_engine_options(n_runs=R)`` trains R independent models (runs) in the same launches on the same data set.  Run 0
    starts from the module's parameters and shuffles with the global torch RNG, exactly as a one-run object does; run r > 0 starts from
    ``RNNModel``'s initialisation under torch seed ``seed + r`` and shuffles with a generator of its own seeded ``seed + r``.  The
    scaler is shared.  The torch module shows the run chosen by ``select_run`` (run 0 by default)."""

    def __init__(self, model: nn.Module, optim: torch.optim.Optimizer, scaler: StandardScaler,
                 terminal_fn: Callable[[np.ndarray, np.ndarray, np.ndarray], np.ndarray]) -> None:
        super().__init__(model, optim)
        from ..nets import RNNModel
        if not isinstance(model, RNNModel):
            raise NotImplementedError(f"RNNDynamics runs offlinerlkit.nets.RNNModel on the HIP engine, got {type(model).__name__}")
        if type(optim) is not torch.optim.Adam:
            raise NotImplementedError(f"RNNDynamics supports torch.optim.Adam only, got {type(optim).__name__}")
        if len(optim.param_groups) != 1:
            raise NotImplementedError("RNNDynamics supports one parameter group")
        g = optim.param_groups[0]
        if g.get("weight_decay", 0.0) or g.get("amsgrad", False) or g.get("maximize", False):
            raise NotImplementedError("RNNDynamics supports Adam without weight_decay, amsgrad or maximize")
        dims = list(model.hidden_dims)
        if len(set(dims)) != 1:
            raise NotImplementedError(f"the HIP engine supports RNNModel with equal hidden_dims (the residual blocks add their input), got {dims}")
        if not 2 <= len(dims) <= _engine.MAX_HIDDEN + 1:
            raise NotImplementedError(f"the HIP engine supports 2 to {_engine.MAX_HIDDEN + 1} hidden_dims in RNNModel, got {len(dims)}")
        if dims[0] % 4 or not 8 <= dims[0] <= 512:
            raise NotImplementedError(f"the HIP engine supports a hidden width that is a multiple of 4 in [8, 512], got {dims[0]}")
        if not 1 <= model.rnn_num_layers <= 4:
            raise NotImplementedError(f"the HIP engine supports 1 to 4 GRU layers, got {model.rnn_num_layers}")
        if not 0.0 <= float(model.dropout_rate or 0.0) < 1.0:
            raise ValueError(f"dropout_rate must be in [0, 1), got {model.dropout_rate}")
        self.scaler = scaler
        self.terminal_fn = terminal_fn
        self._n_runs, self._seed = 1, 0
        self._cur_run = 0
        self._gens: Optional[List[torch.Generator]] = None      # the epoch-order generators of runs 1 .. R - 1, carried across epochs
        self._eng: Optional[_engine.RnnDynamicsEngine] = None
        self._arena = None
        self._shape = None              # (batch_size, max_seq_len) the engine was built for
        self._state_n: Optional[int] = None     # trajectories of the carried state (reset_state), None: no state

    # a rollout carries this model's recurrent state on the device: RcslPolicy.rollout / rollout_device call reset_state and pass the
    # live trajectory indices to step_state / step_device
    stateful = True

    # ---- engine binding ----
    def set_engine_options(self, n_runs: int = 1, seed: Optional[int] = None) -> None:
        if self._eng is not None:
            raise RuntimeError("set_engine_options before the first train() / learn() / step()")
        if not 1 <= int(n_runs) <= 64:
            raise ValueError(f"n_runs must be in [1, 64], got {n_runs}")
        self._n_runs = int(n_runs)
        self._seed = int(seed) if seed is not None else 0
        self._gens = None

    def _bind(self, rows: int, steps: int, exact: bool = False) -> None:
        """an engine for steps of up to ``rows`` sequences (``exact``: batch_size == rows, as learn_epoch cuts an epoch into
        batch_size rows) of up to ``steps`` time steps; an engine that is too small is rebuilt and its state (every run's three
        blocks and the step count) carried over"""
        old = self._shape if self._eng is not None else (0, 0)
        if self._eng is not None and steps <= old[1] and (rows == old[0] if exact else rows <= old[0]):
            return
        shape = (int(rows) if exact else max(int(rows), old[0]), max(int(steps), old[1]))
        R = self._n_runs
        carried = None
        if self._eng is not None:
            carried = ([[self._eng.get(which, r) for which in range(3)] for r in range(R)], self._eng.step_count)
            self._unbind()
        dev = self._device()
        m, g = self.model, self.optim.param_groups[0]
        cfg = _engine.default_rnn_config(input_dim=m.input_dim, output_dim=m.output_dim, hidden=m.hidden_dims,
                                         rnn_num_layers=m.rnn_num_layers, dropout_rate=float(m.dropout_rate or 0.0),
                                         batch_size=shape[0], max_seq_len=shape[1], lr=float(g["lr"]), adam_beta1=float(g["betas"][0]),
                                         adam_beta2=float(g["betas"][1]), adam_eps=float(g["eps"]), n_runs=R, device=dev.index,
                                         seed=self._seed)
        self._arena = torch.zeros(R * _engine.rnn_run_floats(cfg), dtype=torch.float32, device=dev)
        cfg.external_arena = self._arena.data_ptr()
        torch.cuda.synchronize(dev)
        self._eng = _engine.RnnDynamicsEngine(cfg)
        self._shape = shape
        self._state_n = None            # (the carried state lived in the old engine)
        for r in range(R):
            if carried is not None:
                for which in range(3):
                    self._eng.set(which, carried[0][r][which], r)
                continue
            src = m.state_dict() if r == 0 else _fresh_rnn_params(m, self._seed + r)
            self._eng.set_params({k: v.detach().cpu().numpy() for k, v in src.items()}, r)
        if carried is not None:
            self._eng.step_count = carried[1]
        m.to(dev)
        m.device = dev
        run, self._cur_run = self._cur_run, -1
        self.select_run(run)

    def select_run(self, run: int) -> None:
        """point the torch module (forward, state_dict, save, load, step on one set of windows) at run ``run``"""
        if not 0 <= int(run) < self._n_runs:
            raise ValueError(f"run {run} out of range ({self._n_runs} runs)")
        if self._eng is None:
            if run != 0:
                raise RuntimeError("select_run before the engine exists: only run 0")
            return
        if run == self._cur_run:
            return
        torch.cuda.synchronize(self._arena.device)
        self._alias_params(int(run) * self._eng.floats, self._eng.tensors())
        self._cur_run = int(run)

    def _drain(self) -> None:
        torch.cuda.synchronize(self._arena.device)

    @staticmethod
    def _host(x) -> np.ndarray:
        return np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32)

    # ---- reference API ----
    @torch.no_grad()
    def step(self, obss: np.ndarray, actions: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, Dict]:
        """imagine single forward step.  Windows ``(N, T, .)``: the selected run.  Windows ``(R, N, T, .)``: run r on ``obss[r]``, every
        result with a leading R (the scaler is shared, ``terminal_fn`` is applied per run)."""
        inputs = self.scaler.transform(np.concatenate([obss, actions], axis=-1))
        self._bind(1, inputs.shape[-2])
        if inputs.ndim == 4:
            if inputs.shape[0] != self._n_runs:
                raise ValueError(f"windows of {inputs.shape[0]} runs for an object of {self._n_runs}")
            preds = self._eng.forward_runs(self._host(inputs), run=-1)
            next_obss = preds[..., :-1] + obss[:, :, -1]
            rewards = preds[..., -1:]
            terminals = np.stack([self.terminal_fn(obss[r, :, -1], actions[r, :, -1], next_obss[r]) for r in range(self._n_runs)])
            return next_obss, rewards, terminals, {}
        if self._n_runs == 1:
            preds = self._eng.forward(self._host(inputs))
        else:
            preds = self._eng.forward_runs(self._host(inputs), run=self._cur_run)
        next_obss = preds[..., :-1] + obss[:, -1]
        rewards = preds[..., -1:]
        terminals = self.terminal_fn(obss[:, -1], actions[:, -1], next_obss)
        return next_obss, rewards, terminals, {}

    # ---- the carried state: one model step at a time (orl_rnn_state_* of the engine) ----
    @property
    def term_kind(self) -> Optional[int]:
        """the ``TERM_*`` kind of the termination function (utils.termination_fns), None when it is not a fixed row-wise test"""
        from ..utils import termination_fns
        return termination_fns.term_kind(self.terminal_fn)

    def _roll_dims(self, what: str) -> Tuple[int, int]:
        """(obs_dim, act_dim) of the one-step interface: the model predicts [delta obs | reward] from [obs | action]"""
        obs_dim = int(self.model.output_dim) - 1
        act_dim = int(self.model.input_dim) - obs_dim
        if obs_dim < 1 or act_dim < 1:
            raise ValueError(f"{what}: output_dim {self.model.output_dim} must be obs_dim + 1 and input_dim {self.model.input_dim} "
                             f"obs_dim + act_dim with act_dim >= 1")
        if self.scaler is None or self.scaler.mu is None:
            raise RuntimeError(f"{what}: the scaler is not fitted: fit or load it first")
        return obs_dim, act_dim

    def _roll_rows(self, what: str, obs, act, index, lead: int):
        """the refusals of a step's arrays: rank, widths (output_dim == obs_dim + 1), a state to step, the index's length"""
        obs_dim, act_dim = self._roll_dims(what)
        if obs.ndim != lead + 2 or act.ndim != lead + 2 or tuple(obs.shape[:-1]) != tuple(act.shape[:-1]):
            shape = ("R, " if lead else "") + "N, "
            raise ValueError(f"{what}: obs {tuple(obs.shape)} / action {tuple(act.shape)} must be ({shape}obs_dim) / ({shape}act_dim)")
        if int(obs.shape[-1]) + 1 != int(self.model.output_dim):
            raise ValueError(f"{what}: output_dim {self.model.output_dim} != obs_dim + 1 for observations of {int(obs.shape[-1])} columns")
        if int(act.shape[-1]) != act_dim:
            raise ValueError(f"{what}: actions of {int(act.shape[-1])} columns, input_dim - obs_dim = {act_dim}")
        if lead and int(obs.shape[0]) != self._n_runs:
            raise ValueError(f"{what}: rows of {int(obs.shape[0])} runs for an object of {self._n_runs}")
        if self._state_n is None or self._eng is None:
            raise RuntimeError(f"{what}: no carried state: reset_state(n_traj) first")
        n = int(obs.shape[-2])
        if index is not None and (index.ndim != 1 or int(index.shape[0]) != n):
            raise ValueError(f"{what}: index {tuple(index.shape)} must name one trajectory per row ({n},)")
        if n > self._state_n:
            raise ValueError(f"{what}: {n} rows (index of {n}) for a state of {self._state_n} trajectories")

    def reset_state(self, n_traj: int, windows=None) -> None:
        """Start a rollout of ``n_traj`` trajectories: their GRU state, kept on the device, is zero (the reference's ``h_state=None``),
        or with ``windows=(obss, actions)`` of shape ``(n_traj, T, .)`` (``(R, n_traj, T, .)``: one history per run) the state after
        those T steps.  The scaler is read here: fit or load it before."""
        self._roll_dims("reset_state")
        if int(n_traj) < 1:
            raise ValueError(f"reset_state: n_traj {n_traj}")
        T = 1
        if windows is not None:
            obss, actions = (np.asarray(self._host(x)) for x in windows)
            inputs = self.scaler.transform(np.concatenate([obss, actions], axis=-1))
            if inputs.ndim not in (3, 4) or inputs.shape[-3] != int(n_traj) or (inputs.ndim == 4 and inputs.shape[0] != self._n_runs):
                raise ValueError(f"reset_state: windows {tuple(inputs.shape)} must be ({n_traj}, T, .) or ({self._n_runs}, {n_traj}, T, .)")
            T = int(inputs.shape[-2])
        self._bind(1, T)
        self._drain()
        self._eng.set_scaler(self.scaler.mu, self.scaler.std)
        self._eng.state_reset(int(n_traj))
        self._state_n = int(n_traj)
        if windows is not None:
            self._eng.state_prime(self._host(inputs))

    @torch.no_grad()
    def step_state(self, obs: np.ndarray, actions: np.ndarray, index=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, Dict]:
        """one model step from the carried state on numpy rows: obs (N, obs_dim), actions (N, act_dim) of the selected run, or
        (R, N, .) of every run; ``index`` (N,): the trajectory of each row (default 0 .. N - 1).  -> (next_obs, reward (.., N, 1),
        terminals, {}), ``terminal_fn`` applied on the host.  The launches of ``step_device``."""
        obs, actions = self._host(obs), self._host(actions)
        index = None if index is None else np.ascontiguousarray(self._index_host(index), dtype=np.int64)
        runs = obs.ndim == 3
        self._roll_rows("step_state", obs, actions, index, int(runs))
        if index is not None and index.size and (index.min() < 0 or index.max() >= self._state_n):
            raise ValueError(f"step_state: trajectory index out of range ({self._state_n} trajectories)")
        self._drain()
        nxt, rew = self._eng.state_step(obs, actions, index, run=-1 if runs else self._cur_run)
        if runs:
            terminals = np.stack([self.terminal_fn(obs[r], actions[r], nxt[r]) for r in range(self._n_runs)])
        else:
            terminals = self.terminal_fn(obs, actions, nxt)
        return nxt, rew[..., None], terminals, {}

    @staticmethod
    def _index_host(index):
        return index.detach().cpu().numpy() if torch.is_tensor(index) else np.asarray(index)

    def _roll_tensors(self, what: str, obs, action, index, lead: int):
        dev = self._arena.device if self._arena is not None else None
        if dev is None:
            raise RuntimeError(f"{what}: no carried state: reset_state(n_traj) first")
        o = torch.as_tensor(obs, dtype=torch.float32, device=dev).contiguous()
        a = torch.as_tensor(action, dtype=torch.float32, device=dev).contiguous()
        ix = None if index is None else torch.as_tensor(index, dtype=torch.int64, device=dev).contiguous()
        self._roll_rows(what, o, a, ix, lead)
        return o, a, ix

    @torch.no_grad()
    def step_device(self, obs: torch.Tensor, action: torch.Tensor, index=None) -> Tuple[torch.Tensor, torch.Tensor, Dict]:
        """``step_state`` without the termination function, on tensors of the engine's device and without a host copy: obs (N, obs_dim),
        action (N, act_dim), ``index`` (N,) int64 (the live trajectories, e.g. ``TrajStore.live_index()``; distinct and inside the
        state: device indices are not read back, the kernels clamp them) -> (next_obs (N, obs_dim), reward (N,), {}) of the selected
        run.  The termination test is left to the consumer (``TrajStore.append_step`` runs ``term_kind`` on the device)."""
        o, a, ix = self._roll_tensors("step_device", obs, action, index, 0)
        nxt, rew = self._eng.state_step(o, a, ix, run=self._cur_run)
        return nxt, rew, {}

    @torch.no_grad()
    def step_device_runs(self, obs: torch.Tensor, action: torch.Tensor, index=None) -> Tuple[torch.Tensor, torch.Tensor, Dict]:
        """``step_device`` of every run at once: obs (R, N, obs_dim), action (R, N, act_dim), run r on block r; ``index`` (N,) is
        shared by the runs -> (next_obs (R, N, obs_dim), reward (R, N), {})"""
        o, a, ix = self._roll_tensors("step_device_runs", obs, action, index, 1)
        nxt, rew = self._eng.state_step(o, a, ix, run=-1)
        return nxt, rew, {}

    def _load_batch(self, batch) -> int:
        inputs, targets, masks = (self._host(x) for x in batch)
        if not self.model.training and float(self.model.dropout_rate or 0.0) > 0.0:
            raise NotImplementedError("RNNDynamics.learn on a model in eval mode: the engine's training step always applies the dropout")
        self._bind(inputs.shape[0], inputs.shape[1])
        self._eng.load_data(inputs, targets, masks)
        return inputs.shape[0]

    def learn(self, batch) -> float:
        """one step of every run on ``batch``; the selected run's loss"""
        if self._n_runs > 1:
            return float(self.learn_runs(batch)[self._cur_run])
        n = self._load_batch(batch)
        return self._eng.step(np.arange(n))

    def learn_runs(self, batch) -> np.ndarray:
        """one step of every run on ``batch``; the R losses"""
        n = self._load_batch(batch)
        return self._eng.step_runs(np.tile(np.arange(n, dtype=np.int64), (self._n_runs, 1)))

    def _epoch_orders(self, n: int) -> np.ndarray:
        """[R, n]: run 0's order from the global torch RNG (as a one-run object draws it), run r's from its own generator"""
        if self._gens is None:
            self._gens = []
            for r in range(1, self._n_runs):
                g = torch.Generator()
                g.manual_seed(self._seed + r)
                self._gens.append(g)
        return np.stack([rnn_epoch_order(n)] + [rnn_epoch_order(n, g) for g in self._gens])

    def train(self, data, batch_size: int, max_iters: int, logger) -> None:
        self.model.train()
        items = [data[i] for i in range(len(data))]
        inputs, targets, masks = (np.stack([self._host(it[k]) for it in items]) for k in range(3))
        self._bind(int(batch_size), inputs.shape[1], exact=True)
        self._eng.load_data(inputs, targets, masks)
        R = self._n_runs
        for it in range(max_iters):
            if R == 1:
                for loss in self._eng.learn_epoch(rnn_epoch_order(len(items))):
                    logger.logkv_mean("loss/model", float(loss))
            else:
                for losses in self._eng.learn_epoch_runs(self._epoch_orders(len(items))):
                    logger.logkv_mean("loss/model", float(np.mean(losses, dtype=np.float64)))
                    for r in range(R):
                        logger.logkv_mean(f"run{r}/loss/model", float(losses[r]))
            logger.set_timestep(it)
            logger.dumpkvs(exclude=["policy_training_progress"])
        self.save(logger.model_dir)
        if R > 1:
            names = list(self.model.state_dict().keys())
            for r in range(1, R):
                params = self._eng.get_params(r)
                sd = type(self.model.state_dict())((k, torch.from_numpy(params[k].copy())) for k in names)
                torch.save(sd, os.path.join(logger.model_dir, f"dynamics_run{r}.pth"))
        self.model.eval()

    def load(self, load_path: str) -> None:
        self.model.load_state_dict(torch.load(os.path.join(load_path, "dynamics.pth"), map_location=self.model.device))
        self.scaler.load_scaler(load_path)
        if self._eng is not None:
            torch.cuda.synchronize(self._arena.device)


__all__ = ["BaseDynamics", "EnsembleDynamics", "RNNDynamics", "rnn_epoch_order"]

"""Autoregressive behaviour policy (reference: policy/others/autoregressive.py:9-124) on the HIP engine: p(a | s) = prod_j N(a_j | s, a_<j)
from ONE net, [Linear, LeakyReLU(0.01)] x (L + 1) on [obs | act masked to the earlier dimensions | one-hot of the predicted dimension] with
the two outputs (mean, logstd).  ``learn`` is the Gaussian NLL of ``fit`` over the act_dim-fold expanded batch (``ORL_ALGO_AUTOREG``),
``select_action`` the act_dim sequential forward passes of ``forward`` on the device (``orl_autoreg_sample``).  It is what
``RcslPolicy.rollout`` rolls through a dynamics model, and ``RcslPolicyTrainer`` trains it like the return-conditioned policies
(run_regress.py); the return-to-go is accepted and ignored, as in the reference."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn
from torch.distributions import Normal

from .. import _engine
from .base_policy import _adam_hyper
from .rcsl import _EpochPolicy

MAX_ACT_DIM = 32


class _ModelNet(nn.Module):
    """the engine's view of the policy's net: the ``model`` ModuleList under the reference's key prefix, and the device.  (The policy is
    its own module; this holder is what gets deep-copied and re-initialised for the runs r > 0.)"""

    def __init__(self, model: nn.ModuleList, device) -> None:
        super().__init__()
        self.model = model
        self.device = torch.device(device)


class AutoregressivePolicy(_EpochPolicy):
    ALGO = "autoreg"

    def __init__(self, obs_dim: int, act_dim: int, hidden_dims: List[int], lr: float, device="cpu") -> None:
        super().__init__()
        self.obs_dim = int(obs_dim)
        self.act_dim = int(act_dim)
        hidden_dims = [int(h) for h in hidden_dims]
        if not 1 <= len(hidden_dims) <= _engine.MAX_HIDDEN:
            raise NotImplementedError(f"the HIP engine supports 1 to {_engine.MAX_HIDDEN} hidden layers, hidden_dims has {len(hidden_dims)}")
        if not 1 <= self.act_dim <= MAX_ACT_DIM:
            raise NotImplementedError(f"the HIP engine's autoregressive policy supports act_dim up to {MAX_ACT_DIM}, got {act_dim}")
        # input: obs + act + one-hot of the predicted dimension; output: mean and logstd of that dimension
        all_dims = [self.obs_dim + 2 * self.act_dim] + hidden_dims + [2]
        self.model = nn.ModuleList()
        for in_dim, out_dim in zip(all_dims[:-1], all_dims[1:]):
            self.model.append(nn.Linear(in_dim, out_dim))
            self.model.append(nn.LeakyReLU())
        self.rcsl_optim = torch.optim.Adam(self.model.parameters(), lr=lr)
        self.device = device
        self.model = self.model.to(self.device)
        self._dims()

    # -- engine hooks ----------------------------------------------------------------------
    def _dims(self):
        """(obs_dim, act_dim, hidden widths) of ``self.model`` -- or a refusal of what the engine does not implement"""
        _adam_hyper(self.rcsl_optim)
        mods = list(self.model)
        lins = mods[0::2]
        ok = len(mods) >= 4 and len(mods) % 2 == 0 and all(isinstance(m, nn.Linear) and m.bias is not None for m in lins) and \
            all(isinstance(m, nn.LeakyReLU) and float(m.negative_slope) == 0.01 for m in mods[1::2])
        ok = ok and all(a.out_features == b.in_features for a, b in zip(lins[:-1], lins[1:])) and lins[-1].out_features == 2 and \
            lins[0].in_features == self.obs_dim + 2 * self.act_dim
        if not ok:
            raise NotImplementedError("AutoregressivePolicy expects model = [Linear, LeakyReLU(0.01)] x (L + 1) from obs_dim + 2 act_dim "
                                      "inputs to 2 outputs (mean, logstd)")
        hidden = [m.out_features for m in lins[:-1]]
        if len(hidden) > _engine.MAX_HIDDEN:
            raise NotImplementedError(f"the HIP engine supports up to {_engine.MAX_HIDDEN} hidden layers, the model has {len(hidden)}")
        if self.act_dim > MAX_ACT_DIM:
            raise NotImplementedError(f"the HIP engine's autoregressive policy supports act_dim up to {MAX_ACT_DIM}, got {self.act_dim}")
        return self.obs_dim, self.act_dim, hidden

    def _nets(self):
        holder = self.__dict__.get("_holder")
        if holder is None or holder.model is not self.model:
            holder = _ModelNet(self.model, self.device)
            self.__dict__["_holder"] = holder      # (not a registered submodule: state_dict keeps the reference's keys model.<i>.*)
        return {_engine.NET_ACTOR: holder}

    def _optims(self):
        return {_engine.OPT_ACTOR: self.rcsl_optim}

    def _config(self) -> Dict:
        od, ad, hidden = self._dims()
        return dict(obs_dim=od, act_dim=ad, hidden=hidden, actor_lr=float(self.rcsl_optim.param_groups[0]["lr"]))

    # -- training --------------------------------------------------------------------------
    def learn(self, batch: Dict) -> Dict[str, float]:
        """One gradient step on ``{"observations", "actions", "rtgs"}`` ([B, ...] arrays shared by every run or [n_runs, B, ...]); the
        return-to-go is accepted and ignored"""
        return self._step_on(batch, (("observations", "observations", None), ("actions", "actions", None)))

    def fit(self, obs: torch.Tensor, act: torch.Tensor) -> torch.Tensor:
        """the loss ``learn`` minimises, restated in torch on the live parameters (autoregressive.py:64-96) for callers that want the
        number; ``learn`` does not go through it"""
        batch_size = obs.size(0)
        one_hot_all = torch.eye(self.act_dim, device=obs.device)
        one_hot_full = one_hot_all.repeat_interleave(batch_size, dim=0)
        mask = torch.tril(torch.ones((self.act_dim, self.act_dim), device=obs.device)) - one_hot_all      # strictly lower triangle
        act_full = act.repeat(self.act_dim, 1)
        x = torch.cat([obs.repeat(self.act_dim, 1), act_full * mask.repeat_interleave(batch_size, dim=0), one_hot_full], dim=1)
        target = act_full[one_hot_full.bool()].unsqueeze(1)
        for layer in self.model:
            x = layer(x)
        mean, logstd = torch.chunk(x, 2, dim=-1)
        return -Normal(mean, logstd.exp()).log_prob(target).mean()

    # -- sampling --------------------------------------------------------------------------
    def _sample(self, obs: torch.Tensor, eps: torch.Tensor) -> torch.Tensor:
        """``obs`` [n_runs, n, obs_dim], ``eps`` [n_runs, n, act_dim] on the engine's device -> actions [n_runs, n, act_dim]"""
        obs, eps = obs.contiguous(), eps.contiguous()
        out = torch.empty_like(eps)
        torch.cuda.current_stream(obs.device).synchronize()
        self._eng.autoreg_sample(obs.data_ptr(), eps.data_ptr(), n=int(obs.shape[1]), out_ptr=out.data_ptr(), on_device=True)
        return out

    def select_action(self, obs: np.ndarray, rtg=None) -> np.ndarray:
        """Sampled actions for ``obs`` [n, obs_dim], any n (the reference's ``forward`` serves one row: its ``if logstd.exp() == 0`` raises
        on more; batched rows are its row-wise generalisation).  The standard normals are ``torch.randn((n, act_dim))`` on the device's
        torch generator, so ``torch.manual_seed`` reproduces; ``rtg`` is accepted and ignored.  With several runs: the selected run's."""
        return self.select_action_device(torch.as_tensor(np.asarray(obs, dtype=np.float32))).cpu().numpy()

    def select_action_device(self, obs: torch.Tensor) -> torch.Tensor:
        """``select_action`` without the host round trip: ``obs`` [n, obs_dim] (moved to the engine's device when it is elsewhere) ->
        actions [n, act_dim] on the engine's device.  The same ``torch.randn((n, act_dim))`` draw, so under one ``torch.manual_seed`` it
        consumes the stream ``select_action`` consumes; with several runs: the selected run's rows."""
        if self._eng is None:
            self._bind(256)
        dev = self._arena.device
        o = torch.as_tensor(obs, dtype=torch.float32, device=dev).reshape(-1, self.obs_dim)
        eps = torch.randn((o.shape[0], self.act_dim), device=dev)
        R, r = self._n_runs, max(self._cur_run, 0)
        if R > 1:
            eps_all = torch.zeros((R,) + tuple(eps.shape), device=dev)
            eps_all[r] = eps
            return self._sample(o.unsqueeze(0).expand(R, -1, -1), eps_all)[r]
        return self._sample(o.unsqueeze(0), eps.unsqueeze(0))[0]

    def loop_engine(self) -> "_engine.Engine":
        """the engine a device loop samples through (``RcslPolicy.rollout_device(fused=True)``), bound like ``select_action_device`` binds it"""
        if self._eng is None:
            self._bind(256)
        return self._eng

    def select_action_runs(self, obs: np.ndarray, rtg=None) -> np.ndarray:
        """Sampled actions of EVERY run in one call: ``obs`` [n_runs, E, obs_dim] -> [n_runs, E, act_dim]; the normals are one
        ``torch.randn((n_runs, E, act_dim))`` on the device's torch generator"""
        if self._eng is None:
            raise RuntimeError("select_action_runs before the first learn(): no engine is bound yet")
        o = torch.as_tensor(np.asarray(obs, dtype=np.float32), device=self._arena.device)
        if o.dim() != 3 or o.shape[0] != self._n_runs:
            raise ValueError(f"obs: expected [n_runs = {self._n_runs}, E, obs_dim], got {tuple(o.shape)}")
        eps = torch.randn((self._n_runs, o.shape[1], self.act_dim), device=o.device)
        return self._sample(o, eps).cpu().numpy()

    def forward(self, obs: torch.Tensor) -> torch.Tensor:
        return torch.as_tensor(self.select_action(obs.detach().cpu().numpy()), device=obs.device)

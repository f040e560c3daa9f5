"""Actor / critic heads of the hot path (reference: offlinerlkit/modules/{actor,critic,ensemble_critic,dist}_module.py).

As with ``nets``, these describe networks and serve ``select_action`` at evaluation time; the training math
(sampling, log-probabilities, their gradients) lives in the HIP engine (csrc/kernels.h).
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import numpy as np
import torch
import torch.nn as nn

from .nets import EnsembleLinear, MLP  # noqa: F401


def _as_input(x, device) -> torch.Tensor:
    return torch.as_tensor(x, device=device, dtype=torch.float32)


class NormalWrapper(torch.distributions.Normal):
    """Diagonal Gaussian whose log_prob / entropy are summed over the action dimension (dist_module.py:6-14)."""

    def log_prob(self, actions):
        return super().log_prob(actions).sum(-1, keepdim=True)

    def entropy(self):
        return super().entropy().sum(-1)

    def mode(self):
        return self.mean


class TanhNormalWrapper(torch.distributions.Normal):
    """Gaussian squashed by tanh at sampling time (dist_module.py:17-42); log_prob carries the Jacobian term
    -sum log(1 - a^2 + 1e-6)."""

    _EPS = 1e-6

    def log_prob(self, action, raw_action=None):
        if raw_action is None:
            raw_action = self.arctanh(action)
        base = super().log_prob(raw_action).sum(-1, keepdim=True)
        return base - torch.log((1 - action.pow(2)) + self._EPS).sum(-1, keepdim=True)

    def mode(self):
        return torch.tanh(self.mean), self.mean

    def arctanh(self, x):
        return 0.5 * torch.log((1 + x).clamp(min=1e-6) / (1 - x).clamp(min=1e-6))

    def rsample(self):
        raw = super().rsample()
        return torch.tanh(raw), raw


class DiagGaussian(nn.Module):
    """mu = Linear (optionally max_mu * tanh), sigma = exp(clamp(Linear)) or exp(sigma_param (A,1)) (dist_module.py:45-78)."""

    wrapper = NormalWrapper

    def __init__(self, latent_dim, output_dim, unbounded=False, conditioned_sigma=False, max_mu=1.0,
                 sigma_min=-5.0, sigma_max=2.0):
        super().__init__()
        self.mu = nn.Linear(latent_dim, output_dim)
        self._c_sigma = conditioned_sigma
        if conditioned_sigma:
            self.sigma = nn.Linear(latent_dim, output_dim)
        else:
            self.sigma_param = nn.Parameter(torch.zeros(output_dim, 1))
        self._unbounded = unbounded
        self._max = max_mu
        self._sigma_min = sigma_min
        self._sigma_max = sigma_max

    def reset_parameters(self) -> None:
        """the constructor's value of the module's OWN parameter (the Linear children reset themselves): sigma_param = 0"""
        if not self._c_sigma:
            with torch.no_grad():
                self.sigma_param.zero_()

    def _params(self, logits):
        mu = self.mu(logits)
        if not self._unbounded:
            mu = self._max * torch.tanh(mu)
        if self._c_sigma:
            log_sigma = torch.clamp(self.sigma(logits), min=self._sigma_min, max=self._sigma_max)
        else:
            shape = [1] * mu.dim()
            shape[1] = -1
            log_sigma = self.sigma_param.view(shape) + torch.zeros_like(mu)
        return mu, log_sigma

    def forward(self, logits):
        mu, log_sigma = self._params(logits)
        return self.wrapper(mu, log_sigma.exp())

    def get_dist_params(self, logits):
        return self._params(logits)


class TanhDiagGaussian(DiagGaussian):
    """Same parameters, tanh-squashed samples (dist_module.py:95-127)."""

    wrapper = TanhNormalWrapper


class ActorProb(nn.Module):
    """backbone -> dist_net -> distribution (actor_module.py:9-27)."""

    def __init__(self, backbone: nn.Module, dist_net: nn.Module, device: str = "cpu") -> None:
        super().__init__()
        self.device = torch.device(device)
        self.backbone = backbone.to(device)
        self.dist_net = dist_net.to(device)

    def forward(self, obs: Union[np.ndarray, torch.Tensor]):
        return self.dist_net(self.backbone(_as_input(obs, self.device)))


class Actor(nn.Module):
    """Deterministic actor: max_action * tanh(Linear(backbone(obs))) (actor_module.py:30-51)."""

    def __init__(self, backbone: nn.Module, action_dim: int, max_action: float = 1.0, device: str = "cpu") -> None:
        super().__init__()
        self.device = torch.device(device)
        self.backbone = backbone.to(device)
        self.last = nn.Linear(getattr(backbone, "output_dim"), action_dim).to(device)
        self._max = max_action

    def forward(self, obs: Union[np.ndarray, torch.Tensor]) -> torch.Tensor:
        return self._max * torch.tanh(self.last(self.backbone(_as_input(obs, self.device))))


class Critic(nn.Module):
    """Q(s,a) (or V(s) when actions is None): cat -> backbone -> Linear(H,1) (critic_module.py:9-28)."""

    def __init__(self, backbone: nn.Module, device: str = "cpu") -> None:
        super().__init__()
        self.device = torch.device(device)
        self.backbone = backbone.to(device)
        self.last = nn.Linear(getattr(backbone, "output_dim"), 1).to(device)

    def forward(self, obs, actions: Optional[Union[np.ndarray, torch.Tensor]] = None) -> torch.Tensor:
        x = _as_input(obs, self.device)
        if actions is not None:
            x = torch.cat([x, _as_input(actions, self.device).flatten(1)], dim=1)
        return self.last(self.backbone(x))


class RcslModule(nn.Module):
    """Return-conditioned policy network: backbone([obs | rtg]) (modules/rcsl_module.py:8-33).  The backbone is an ``MLP`` built with
    ``output_dim = act_dim``: its last Linear is the output layer, so the state_dict keys are ``backbone.model.{0,2,...,2L}.*``."""

    def __init__(self, backbone: nn.Module, device: str = "cpu") -> None:
        super().__init__()
        self.device = torch.device(device)
        self.backbone = backbone.to(device)

    def forward(self, obs: Union[np.ndarray, torch.Tensor], rtg: Union[np.ndarray, torch.Tensor]) -> torch.Tensor:
        obs = _as_input(obs, self.device)
        rtg = _as_input(rtg, self.device)
        if rtg.dim() == 1:
            rtg = rtg.unsqueeze(-1)
        return self.backbone(torch.cat([obs, rtg], dim=-1))


class RcslGaussianModule(nn.Module):
    """Return-conditioned Gaussian policy network: dist_net(backbone([obs | rtg])) (modules/rcsl_gauss_module.py:12-54).  ``forward``
    returns the ``NormalWrapper`` (scale = exp of the clamped head output), ``get_dist_params`` the pair (mu, that same clamped output),
    which ``RcslGaussianPolicy.learn`` reads as a log-variance: the reference's asymmetry, kept."""

    def __init__(self, backbone: nn.Module, dist_net: DiagGaussian, device: str = "cpu") -> None:
        super().__init__()
        self.device = torch.device(device)
        self.backbone = backbone.to(device)
        self.dist_net = dist_net.to(device)

    def _latent(self, obs, rtg) -> torch.Tensor:
        obs = _as_input(obs, self.device)
        rtg = _as_input(rtg, self.device)
        if rtg.dim() == 1:
            rtg = rtg.unsqueeze(-1)
        return self.backbone(torch.cat([obs, rtg], dim=-1))

    def forward(self, obs: Union[np.ndarray, torch.Tensor], rtg: Union[np.ndarray, torch.Tensor]) -> torch.distributions.Normal:
        return self.dist_net(self._latent(obs, rtg))

    def get_dist_params(self, obs: Union[np.ndarray, torch.Tensor], rtg: Union[np.ndarray, torch.Tensor]):
        return self.dist_net.get_dist_params(self._latent(obs, rtg))


class EnsembleCritic(nn.Module):
    """K parallel critic MLPs built from EnsembleLinear; output (K, B, 1) (ensemble_critic_module.py:11-44)."""

    def __init__(self, obs_dim: int, action_dim: int, hidden_dims: Sequence[int], activation=nn.ReLU,
                 num_ensemble: int = 10, device: str = "cpu") -> None:
        super().__init__()
        dims = [obs_dim + action_dim] + list(hidden_dims)
        layers = []
        for d_in, d_out in zip(dims, dims[1:]):
            layers += [EnsembleLinear(d_in, d_out, num_ensemble), activation()]
        layers.append(EnsembleLinear(dims[-1], 1, num_ensemble))
        self.device = torch.device(device)
        self.model = nn.Sequential(*layers).to(device)
        self._num_ensemble = num_ensemble
        self.obs_dim, self.action_dim, self.hidden_dims = obs_dim, action_dim, list(hidden_dims)

    def forward(self, obs, actions=None) -> torch.Tensor:
        x = _as_input(obs, self.device)
        if actions is not None:
            x = torch.cat([x, _as_input(actions, self.device)], dim=-1)
        return self.model(x)


# ---- dynamics ensemble (reference: modules/dynamics_module.py:9-119) ----

class Swish(nn.Module):
    """x * sigmoid(x) (dynamics_module.py:9-16)"""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x * torch.sigmoid(x)


def soft_clamp(x: torch.Tensor, _min: Optional[torch.Tensor] = None, _max: Optional[torch.Tensor] = None) -> torch.Tensor:
    """clamp keeping a gradient (dynamics_module.py:19-29): max - softplus(max - x), then min + softplus(x - min)"""
    if _max is not None:
        x = _max - torch.nn.functional.softplus(_max - x)
    if _min is not None:
        x = _min + torch.nn.functional.softplus(x - _min)
    return x


class EnsembleDynamicsModel(nn.Module):
    """Probabilistic ensemble of ``num_ensemble`` Swish MLPs (dynamics_module.py:32-119); the output layer gives [mean | logvar] of
    (delta obs, reward).  Same parameter registration order (state_dict keys) and, under the same torch seed, the same initial
    parameters as the reference.  Training runs in the HIP engine (``offlinerlkit.dynamics.EnsembleDynamics``), which re-points these
    parameters at its arena; ``forward`` stays a torch function for evaluation."""

    def __init__(self, obs_dim: int, action_dim: int, hidden_dims: Sequence[int], num_ensemble: int = 7, num_elites: int = 5,
                 activation=Swish, weight_decays: Optional[Sequence[float]] = None, with_reward: bool = True,
                 device: str = "cpu") -> None:
        super().__init__()
        self.num_ensemble = num_ensemble
        self.num_elites = num_elites
        self._with_reward = with_reward
        self.device = torch.device(device)
        if activation is not Swish:
            raise NotImplementedError("the engine's dynamics kernels implement the Swish activation only")
        self.activation = activation()
        if weight_decays is None:
            weight_decays = [0.0] * (len(hidden_dims) + 1)
        assert len(weight_decays) == (len(hidden_dims) + 1)
        self.obs_dim, self.action_dim = int(obs_dim), int(action_dim)
        self.hidden_dims = [int(h) for h in hidden_dims]
        self.weight_decays = [float(w) for w in weight_decays]
        dims = [obs_dim + action_dim] + list(hidden_dims)
        self.backbones = nn.ModuleList([EnsembleLinear(i, o, num_ensemble, w) for i, o, w in zip(dims[:-1], dims[1:], weight_decays[:-1])])
        self.output_layer = EnsembleLinear(dims[-1], 2 * (obs_dim + self._with_reward), num_ensemble, weight_decays[-1])
        self.register_parameter("max_logvar", nn.Parameter(torch.ones(obs_dim + self._with_reward) * 0.5, requires_grad=True))
        self.register_parameter("min_logvar", nn.Parameter(torch.ones(obs_dim + self._with_reward) * -10, requires_grad=True))
        self.register_parameter("elites", nn.Parameter(torch.tensor(list(range(0, self.num_elites))), requires_grad=False))
        self.to(self.device)

    def forward(self, obs_action):
        obs_action = torch.as_tensor(obs_action, dtype=torch.float32).to(self.device)
        output = obs_action
        for layer in self.backbones:
            output = self.activation(layer(output))
        mean, logvar = torch.chunk(self.output_layer(output), 2, dim=-1)
        logvar = soft_clamp(logvar, self.min_logvar, self.max_logvar)
        return mean, logvar

    def load_save(self) -> None:
        for layer in self.backbones:
            layer.load_save()
        self.output_layer.load_save()

    def update_save(self, indexes) -> None:
        for layer in self.backbones:
            layer.update_save(indexes)
        self.output_layer.update_save(indexes)

    def get_decay_loss(self) -> torch.Tensor:
        decay_loss = 0
        for layer in self.backbones:
            decay_loss += layer.get_decay_loss()
        decay_loss += self.output_layer.get_decay_loss()
        return decay_loss

    def set_elites(self, indexes) -> None:
        assert len(indexes) <= self.num_ensemble and max(indexes) < self.num_ensemble
        self.register_parameter("elites", nn.Parameter(torch.tensor(list(indexes), device=self.device), requires_grad=False))

    def random_elite_idxs(self, batch_size: int) -> np.ndarray:
        return np.random.choice(self.elites.data.cpu().numpy(), size=batch_size)

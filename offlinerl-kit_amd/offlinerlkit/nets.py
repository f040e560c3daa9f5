"""Backbone networks of the hot path (reference: offlinerlkit/nets/mlp.py:9-33, nets/ensemble_linear.py:9-41).

These torch modules only DESCRIBE a network (shapes, initial weights, eval-time forward for
``select_action``).  Training never runs through them: an engine-backed policy copies their
parameters into the HIP engine's arena and re-points ``param.data`` at views of that arena.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch
import torch.nn as nn


class MLP(nn.Module):
    """[Linear, activation(, Dropout)] x len(hidden_dims) (+ optional output Linear).
    ``self.model`` is an ``nn.Sequential`` so state_dict keys are ``model.<2*i>.{weight,bias}`` like the reference."""

    def __init__(self, input_dim: int, hidden_dims: Sequence[int], output_dim: Optional[int] = None,
                 activation=nn.ReLU, dropout_rate: Optional[float] = None) -> None:
        super().__init__()
        widths = [int(input_dim)] + [int(h) for h in hidden_dims]
        layers: List[nn.Module] = []
        for fan_in, fan_out in zip(widths, widths[1:]):
            layers.append(nn.Linear(fan_in, fan_out))
            layers.append(activation())
            if dropout_rate is not None:
                layers.append(nn.Dropout(p=dropout_rate))
        self.output_dim = widths[-1]
        if output_dim is not None:
            layers.append(nn.Linear(widths[-1], int(output_dim)))
            self.output_dim = int(output_dim)
        self.activation_cls = activation
        self.dropout_rate = dropout_rate
        self.model = nn.Sequential(*layers)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.model(x)

    def linear_layers(self) -> List[nn.Linear]:
        return [m for m in self.model if isinstance(m, nn.Linear)]


class EnsembleLinear(nn.Module):
    """K independent affine maps evaluated together: weight (K, in, out), bias (K, 1, out); y = x @ W + b.
    A 2-D input is shared by every member.  ``saved_weight`` / ``saved_bias`` are the reference's shadow copies
    (ensemble_linear.py:25-26): registered so state_dict keys match, never trained."""

    def __init__(self, input_dim: int, output_dim: int, num_ensemble: int, weight_decay: float = 0.0) -> None:
        super().__init__()
        self.num_ensemble = num_ensemble
        self.weight_decay = weight_decay
        self.input_dim = input_dim
        self.weight = nn.Parameter(torch.zeros(num_ensemble, input_dim, output_dim))
        self.bias = nn.Parameter(torch.zeros(num_ensemble, 1, output_dim))
        self.saved_weight = nn.Parameter(torch.zeros(num_ensemble, input_dim, output_dim))
        self.saved_bias = nn.Parameter(torch.zeros(num_ensemble, 1, output_dim))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        """the constructor's initialisation again (ensemble_linear.py:21-26): trunc_normal(std = 1 / (2 sqrt(in))) weights, zero
        biases, shadow copies equal to them -- what building the layer under another seed gives (runs r > 0 of a multi-run policy)"""
        with torch.no_grad():
            nn.init.trunc_normal_(self.weight, std=1.0 / (2.0 * self.input_dim ** 0.5))
            self.bias.zero_()
            self.saved_weight.copy_(self.weight)
            self.saved_bias.copy_(self.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() == 2:
            y = torch.einsum("ij,bjk->bik", x, self.weight)
        else:
            y = torch.bmm(x, self.weight)
        return y + self.bias

    def load_save(self) -> None:
        self.weight.data.copy_(self.saved_weight.data)
        self.bias.data.copy_(self.saved_bias.data)

    def update_save(self, indexes) -> None:
        self.saved_weight.data[indexes] = self.weight.data[indexes]
        self.saved_bias.data[indexes] = self.bias.data[indexes]

    def get_decay_loss(self) -> torch.Tensor:
        return self.weight_decay * 0.5 * (self.weight ** 2).sum()


class VAE(nn.Module):
    """Vanilla conditional VAE, MCQ's behaviour policy (reference: offlinerlkit/nets/vae.py:8-66): encoder e1, e2 -> mean, log_std
    (clamped to [-4, 15]); decoder d1, d2, d3 -> max_action * tanh; ``decode`` without a latent samples N(0, 1) clipped to +-0.5.
    As with the other nets this describes the parameters and serves evaluation; MCQPolicy.learn runs in the HIP engine."""

    def __init__(self, input_dim: int, output_dim: int, hidden_dim: int, latent_dim: int, max_action, device: str = "cpu") -> None:
        super().__init__()
        self.e1 = nn.Linear(input_dim + output_dim, hidden_dim)
        self.e2 = nn.Linear(hidden_dim, hidden_dim)
        self.mean = nn.Linear(hidden_dim, latent_dim)
        self.log_std = nn.Linear(hidden_dim, latent_dim)
        self.d1 = nn.Linear(input_dim + latent_dim, hidden_dim)
        self.d2 = nn.Linear(hidden_dim, hidden_dim)
        self.d3 = nn.Linear(hidden_dim, output_dim)
        self.max_action = max_action
        self.latent_dim = latent_dim
        self.device = torch.device(device)
        self.to(device=self.device)

    def forward(self, obs: torch.Tensor, action: torch.Tensor):
        z = torch.relu(self.e1(torch.cat([obs, action], 1)))
        z = torch.relu(self.e2(z))
        mean = self.mean(z)
        std = torch.exp(self.log_std(z).clamp(-4, 15))
        z = mean + std * torch.randn_like(std)
        return self.decode(obs, z), mean, std

    def decode(self, obs: torch.Tensor, z=None) -> torch.Tensor:
        if z is None:
            z = torch.randn((obs.shape[0], self.latent_dim)).to(self.device).clamp(-0.5, 0.5)
        a = torch.relu(self.d1(torch.cat([obs, z], 1)))
        a = torch.relu(self.d2(a))
        return self.max_action * torch.tanh(self.d3(a))


# ---- the diffusion behaviour policy's noise-prediction net (reference: offlinerlkit/nets/unet.py) ---------------------------------
# Thin torch modules whose constructor signatures, parameter registration order (hence state_dict keys and, under one torch seed, the
# initial values) and conv weight shapes [out, in, k] are the reference's.  Their ``forward`` serves CPU checks and the stock-torch
# baseline; DiffusionBC trains and samples on the HIP engine (csrc/diffusion.hip), which keeps the centre taps only.

class SinusoidalPosEmb(nn.Module):
    """t [B] -> [sin(t f_j) | cos(t f_j)] [B, dim], f_j = exp(-j ln(10000) / (dim / 2 - 1))"""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        half = self.dim // 2
        freq = torch.exp(torch.arange(half, device=x.device) * -(math.log(10000) / (half - 1)))
        arg = x[:, None] * freq[None, :]
        return torch.cat((arg.sin(), arg.cos()), dim=-1)


class Conv1dBlock(nn.Module):
    """Conv1d(k, padding k // 2) -> GroupNorm -> Mish, as ``self.block``"""

    def __init__(self, inp_channels, out_channels, kernel_size, n_groups=8):
        super().__init__()
        self.block = nn.Sequential(nn.Conv1d(inp_channels, out_channels, kernel_size, padding=kernel_size // 2),
                                   nn.GroupNorm(n_groups, out_channels), nn.Mish())

    def forward(self, x):
        return self.block(x)


class ConditionalResidualBlock1D(nn.Module):
    """two Conv1dBlocks with a FiLM (per-channel scale and bias from ``cond_encoder(cond)``) between them and a residual path
    (a 1x1 conv when the channel counts differ)"""

    def __init__(self, in_channels, out_channels, cond_dim, kernel_size=3, n_groups=8):
        super().__init__()
        self.blocks = nn.ModuleList([Conv1dBlock(in_channels, out_channels, kernel_size, n_groups=n_groups),
                                     Conv1dBlock(out_channels, out_channels, kernel_size, n_groups=n_groups)])
        self.out_channels = out_channels
        self.cond_encoder = nn.Sequential(nn.Mish(), nn.Linear(cond_dim, 2 * out_channels), nn.Unflatten(-1, (-1, 1)))
        self.residual_conv = nn.Conv1d(in_channels, out_channels, 1) if in_channels != out_channels else nn.Identity()

    def forward(self, x, cond):
        """x [B, in_channels, T], cond [B, cond_dim] -> [B, out_channels, T]"""
        film = self.cond_encoder(cond).reshape(cond.shape[0], 2, self.out_channels, 1)
        y = film[:, 0] * self.blocks[0](x) + film[:, 1]
        return self.blocks[1](y) + self.residual_conv(x)


class ConditionalUnet1D(nn.Module):
    """The reference's 1-D U-Net without its (commented-out) down / up sampling: two residual blocks per level on the way down, two in
    the middle, two per level on the way up over [x | skip], then Conv1dBlock + 1x1 conv.  Every block is conditioned on
    [step encoder(t) | global_cond]."""

    def __init__(self, input_dim, global_cond_dim, diffusion_step_embed_dim=256, down_dims=[256, 512, 1024], kernel_size=5, n_groups=8):
        super().__init__()
        dims = [input_dim] + list(down_dims)
        dsed = diffusion_step_embed_dim
        cond_dim = dsed + global_cond_dim
        pairs = list(zip(dims[:-1], dims[1:]))

        def block(cin, cout):
            return ConditionalResidualBlock1D(cin, cout, cond_dim=cond_dim, kernel_size=kernel_size, n_groups=n_groups)

        # construction order = the order the reference draws its initial values in; attribute order = its state_dict order
        step_encoder = nn.Sequential(SinusoidalPosEmb(dsed), nn.Linear(dsed, 4 * dsed), nn.Mish(), nn.Linear(4 * dsed, dsed))
        self.mid_modules = nn.ModuleList([block(dims[-1], dims[-1]), block(dims[-1], dims[-1])])
        down = nn.ModuleList([nn.ModuleList([block(cin, cout), block(cout, cout)]) for cin, cout in pairs])
        up = nn.ModuleList([nn.ModuleList([block(2 * cout, cin), block(cin, cin)]) for cin, cout in reversed(pairs[1:])])
        final = nn.Sequential(Conv1dBlock(down_dims[0], down_dims[0], kernel_size=kernel_size), nn.Conv1d(down_dims[0], input_dim, 1))
        self.diffusion_step_encoder = step_encoder
        self.up_modules = up
        self.down_modules = down
        self.final_conv = final

    def forward(self, sample, timestep, global_cond=None):
        """sample [B, T, input_dim], timestep [B] or a scalar, global_cond [B, global_cond_dim] -> [B, T, input_dim]"""
        x = sample.moveaxis(-1, -2)
        t = timestep
        if not torch.is_tensor(t):
            t = torch.tensor([t], dtype=torch.long, device=x.device)
        elif t.dim() == 0:
            t = t[None].to(x.device)
        emb = self.diffusion_step_encoder[0](t.expand(x.shape[0])).to(x.dtype)       # (float32 in use; float64 nets are for checks)
        cond = self.diffusion_step_encoder[1:](emb)
        if global_cond is not None:
            cond = torch.cat([cond, global_cond], dim=-1)
        skips = []
        for first, second in self.down_modules:
            x = second(first(x, cond), cond)
            skips.append(x)
        for m in self.mid_modules:
            x = m(x, cond)
        for first, second in self.up_modules:
            x = second(first(torch.cat((x, skips.pop()), dim=1), cond), cond)
        return self.final_conv(x).moveaxis(-1, -2)


class Swish(nn.Module):
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x * torch.sigmoid(x)


def soft_clamp(x: torch.Tensor, _min=None, _max=None) -> torch.Tensor:
    """clamp with a softplus knee on either side, so the gradient never vanishes"""
    if _max is not None:
        x = _max - nn.functional.softplus(_max - x)
    if _min is not None:
        x = _min + nn.functional.softplus(x - _min)
    return x


class ResBlock(nn.Module):
    """LayerNorm([x +] dropout(activation(Linear(x)))); state_dict keys ``linear.*`` and ``layer_norm.*`` (reference: nets/rnn.py)"""

    def __init__(self, input_dim: int, output_dim: int, activation: Optional[nn.Module] = None, layer_norm: bool = True,
                 with_residual: bool = True, dropout: Optional[float] = 0.1) -> None:
        super().__init__()
        self.linear = nn.Linear(input_dim, output_dim)
        self.activation = activation if activation is not None else Swish()
        self.layer_norm = nn.LayerNorm(output_dim) if layer_norm else None
        self.dropout = nn.Dropout(dropout) if dropout else None
        self.with_residual = with_residual

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.activation(self.linear(x))
        if self.dropout is not None:
            y = self.dropout(y)
        if self.with_residual:
            y = x + y
        return y if self.layer_norm is None else self.layer_norm(y)


class RNNModel(nn.Module):
    """The sequence model of ``RNNDynamics`` (reference: nets/rnn.py): an ``nn.GRU`` over the input sequence beside a ResBlock of the
    same input (no residual), both merged by ``swish(Linear(2H -> H))``, then ``len(hidden_dims) - 1`` residual ResBlocks and a Linear
    head, applied to every time step.  ``forward`` takes ``[batch, T, input_dim]`` and returns ``([batch, T, output_dim], h_state)``.
    It computes in the parameters' dtype (float32 unless the module was converted)."""

    def __init__(self, input_dim: int, output_dim: int, hidden_dims: Sequence[int] = (200, 200, 200, 200), rnn_num_layers: int = 3,
                 dropout_rate: float = 0.1, device: str = "cpu") -> None:
        super().__init__()
        self.input_dim = int(input_dim)
        self.hidden_dims = [int(h) for h in hidden_dims]
        self.output_dim = int(output_dim)
        self.rnn_num_layers = int(rnn_num_layers)
        self.dropout_rate = dropout_rate
        self.device = torch.device(device)
        widths = self.hidden_dims
        self.activation = Swish()
        self.rnn_layer = nn.GRU(input_size=self.input_dim, hidden_size=widths[0], num_layers=self.rnn_num_layers, batch_first=True)
        self.input_layer = ResBlock(self.input_dim, widths[0], dropout=dropout_rate, with_residual=False)
        self.backbones = nn.ModuleList([ResBlock(a, b, dropout=dropout_rate) for a, b in zip(widths[:-1], widths[1:])])
        self.merge_layer = nn.Linear(widths[0] + widths[-1], widths[0])
        self.output_layer = nn.Linear(widths[-1], self.output_dim)
        self.to(self.device)

    def forward(self, input, h_state=None):
        w = self.output_layer.weight
        x = torch.as_tensor(input, dtype=w.dtype).to(w.device)
        batch, steps = x.shape[0], x.shape[1]
        seq, h_state = self.rnn_layer(x, h_state)
        flat = x.reshape(batch * steps, self.input_dim)
        y = torch.cat([self.input_layer(flat), seq.reshape(batch * steps, self.hidden_dims[0])], dim=-1)
        y = self.activation(self.merge_layer(y))
        for block in self.backbones:
            y = block(y)
        return self.output_layer(y).view(batch, steps, self.output_dim), h_state

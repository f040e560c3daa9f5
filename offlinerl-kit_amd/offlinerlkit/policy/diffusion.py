"""DiffusionBC, the diffusion behaviour policy of the MBRCSL pipeline (reference: policy/others/diffusion.py) on the HIP engine.

The reference builds a ``ConditionalUnet1D`` noise-prediction net and trains it with three pieces of ``diffusers``: a DDPM scheduler
(squared-cosine betas, clipped x0, epsilon prediction), an EMA of the weights (power 0.75) and a cosine learning-rate schedule with 500
warm-up steps.  That package is not a dependency here: the three are a few lines of arithmetic each, restated below (``ddpm_schedule``,
``lr_table``, ``ema_decay``) exactly as the project's DESIGN.md fixes them.

The policy only ever calls the net with a sequence of length 1, where each Conv1d(k, padding k // 2) reads its centre tap and the
U-Net is a FiLM-conditioned residual MLP.  Training (``train``) and sampling (``select_action``) run on ``orl_diffusion_*``
(csrc/diffusion.hip); ``noise_pred_net`` / ``ema_noise_pred_net`` are torch modules that hold the reference-shaped state_dict for
checkpoints.  AdamW's decay factor 1 - lr * 1e-6 rounds to 1.0f for every lr <= 1e-4, so the optimizer is Adam and the off-centre
conv taps, whose gradient is exactly zero, keep their initial values on the host and are written into the checkpoints."""
from __future__ import annotations

import copy
import math
import os
from typing import Optional

import numpy as np
import torch

from .. import _engine
from ..nets import ConditionalUnet1D

LR_MAX, WEIGHT_DECAY, WARMUP_STEPS = 1e-4, 1e-6, 500
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8


def ddpm_schedule(N: int):
    """-> (betas, alphas_cumprod float32 [N], coef float32 [N, 5]).  betas: squared-cosine, capped at 0.999, float64 then float32.
    coef[t] = (sqrt(acp_t), sqrt(1 - acp_t), c0, c1, sigma) of the sampling update
    x <- c0 clip((x - sqrt(1 - acp_t) e) / sqrt(acp_t), -1, 1) + c1 x + sigma z, in float32; sigma is 0 at t = 0."""
    def abar(u):
        return math.cos((u + 0.008) / 1.008 * math.pi / 2) ** 2
    betas = np.array([min(1.0 - abar((i + 1) / N) / abar(i / N), 0.999) for i in range(N)], dtype=np.float64).astype(np.float32)
    acp = np.cumprod(np.float32(1.0) - betas, dtype=np.float32)
    one = np.float32(1.0)
    coef = np.zeros((N, 5), np.float32)
    for t in range(N):
        a, ap = acp[t], (acp[t - 1] if t > 0 else one)
        at = a / ap
        coef[t, 0] = np.sqrt(a)
        coef[t, 1] = np.sqrt(one - a)
        coef[t, 2] = np.sqrt(ap) * (one - at) / (one - a)
        coef[t, 3] = np.sqrt(at) * (one - ap) / (one - a)
        if t > 0:
            coef[t, 4] = np.sqrt(max((one - ap) / (one - a) * (one - at), np.float32(1e-20)))
    return betas, acp, coef


def lr_table(total_steps: int, warmup: int = WARMUP_STEPS, lr_max: float = LR_MAX) -> np.ndarray:
    """the learning rate of optimizer step k (0-based), float64 [total_steps]: linear warm-up, then half a cosine down to 0"""
    T = max(int(total_steps), 1)
    tab = np.empty(T, np.float64)
    for k in range(T):
        if k < warmup:
            tab[k] = lr_max * (k / warmup)
        else:
            tab[k] = lr_max * max(0.0, 0.5 * (1.0 + math.cos(math.pi * (k - warmup) / max(1, T - warmup))))
    return tab


def ema_decay(k: int) -> float:
    """the EMA decay applied after optimizer step k (0-based)"""
    s = max(0, k - 1)
    return 0.0 if s <= 0 else min(1.0 - (1.0 + s) ** -0.75, 0.9999)


def _dataset_arrays(dataset):
    """(obs [n, obs_dim], act [n, act_dim]) from a DeviceBuffer (returned as is), a pair of arrays, or an indexable dataset of
    {"obs", "action"} items"""
    if isinstance(dataset, _engine.DeviceBuffer):
        return dataset
    if isinstance(dataset, (tuple, list)) and len(dataset) == 2 and hasattr(dataset[0], "shape"):
        return np.asarray(dataset[0], np.float32), np.asarray(dataset[1], np.float32)
    items = [dataset[i] for i in range(len(dataset))]
    return (np.stack([np.asarray(it["obs"], np.float32) for it in items]),
            np.stack([np.asarray(it["action"], np.float32) for it in items]))


class DiffusionBC:
    device_frozen_noise = True      # RcslPolicy.rollout_device: sample_init_noise + select_action_device(obs, init_noise) stay in HBM

    def __init__(self, config, dataset, logger):
        """config: act_dim, obs_dim, num_epochs, num_diffusion_iters, batch_size, save_ckpt_freq, device, path; num_workers is
        ignored; spectral_norm=True is refused.  Optional, for nets other than the default: diffusion_step_embed_dim, down_dims,
        kernel_size, n_groups, seed."""
        self.c = config
        self.dataset = dataset
        self.logger = logger
        self.device = config.device
        if getattr(config, "spectral_norm", False):
            raise NotImplementedError("DiffusionBC(spectral_norm=True) is not implemented by the HIP engine")
        if int(getattr(config, "n_runs", 1)) != 1:
            raise NotImplementedError("DiffusionBC: one run per policy (n_runs > 1 is not supported by orl_diffusion)")
        self.net_kwargs = dict(diffusion_step_embed_dim=int(getattr(config, "diffusion_step_embed_dim", 256)),
                               down_dims=[int(h) for h in getattr(config, "down_dims", [256, 512, 1024])],
                               kernel_size=int(getattr(config, "kernel_size", 5)), n_groups=int(getattr(config, "n_groups", 8)))
        if self.net_kwargs["kernel_size"] % 2 == 0:
            raise NotImplementedError("DiffusionBC: kernel_size must be odd (at sequence length 1 the centre tap is the layer)")
        if any(h % self.net_kwargs["n_groups"] for h in self.net_kwargs["down_dims"]):
            raise NotImplementedError("DiffusionBC: every channel count must be a multiple of n_groups")
        if self.net_kwargs["down_dims"][0] % 8:
            raise NotImplementedError("DiffusionBC: down_dims[0] must be a multiple of 8 (final_conv's norm is GroupNorm(8) whatever n_groups is)")
        # AdamW(weight_decay=1e-6) multiplies by 1 - lr * wd, which is 1.0f for every lr of the schedule: the optimizer is Adam
        assert np.float32(1.0 - LR_MAX * WEIGHT_DECAY) == np.float32(1.0)
        self.act_dim, self.obs_dim = int(config.act_dim), int(config.obs_dim)
        self.noise_pred_net = ConditionalUnet1D(input_dim=self.act_dim, global_cond_dim=self.obs_dim, **self.net_kwargs)
        self.ema_noise_pred_net = None
        data = _dataset_arrays(dataset)
        self._n = int(data.size()) if isinstance(data, _engine.DeviceBuffer) else int(len(data[0]))
        self._data = data
        self.steps_per_epoch = -(-self._n // int(config.batch_size))
        self.total_steps = self.steps_per_epoch * int(config.num_epochs)
        self.betas, self.alphas_cumprod, self.ddpm_coef = ddpm_schedule(int(config.num_diffusion_iters))
        self.lr_table = lr_table(self.total_steps)
        self.start_epoch = 0
        self._eng: Optional[_engine.Diffusion] = None
        self._ema_sd = None             # the EMA weights as a state_dict (after train() or load_checkpoint(final=True))

    # -- engine ------------------------------------------------------------------------------
    def _torch_device(self) -> torch.device:
        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise RuntimeError(f"DiffusionBC trains and samples on the HIP engine: config.device must be a GPU, got {self.device!r}")
        return torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())

    def _engine(self) -> _engine.Diffusion:
        if self._eng is None:
            dev = self._torch_device()
            cfg = _engine.default_diffusion_config(
                obs_dim=self.obs_dim, act_dim=self.act_dim, step_embed_dim=self.net_kwargs["diffusion_step_embed_dim"],
                down_dims=self.net_kwargs["down_dims"], kernel_size=self.net_kwargs["kernel_size"], n_groups=self.net_kwargs["n_groups"],
                num_diffusion_iters=int(self.c.num_diffusion_iters), batch_size=int(self.c.batch_size),
                adam_beta1=ADAM_BETAS[0], adam_beta2=ADAM_BETAS[1], adam_eps=ADAM_EPS, device=dev.index,
                seed=int(getattr(self.c, "seed", 0)))
            eng = _engine.Diffusion(cfg)
            eng.set_schedule(self.alphas_cumprod, self.ddpm_coef)
            eng.set_lr(self.lr_table)
            self._table = eng.tensors()
            self._eng = eng
            flat = self.pack(self.noise_pred_net.state_dict())
            eng.set(eng.PARAMS, flat)
            eng.set(eng.EMA, flat if self._ema_sd is None else self.pack(self._ema_sd))
        return self._eng

    def pack(self, state_dict) -> np.ndarray:
        """a reference-shaped state_dict -> the engine's flat block (conv weights: the centre tap)"""
        taps = {name: state_dict[name].detach().cpu().numpy() for name, _, _ in self._table}
        return _engine._flatten(self._table, {k: t[:, :, t.shape[2] // 2] if t.ndim == 3 else t for k, t in taps.items()}, self._eng.floats)

    def unpack(self, flat: np.ndarray, net: torch.nn.Module) -> None:
        """the engine's flat block into ``net``'s parameters; the off-centre taps of ``net`` stay as they are"""
        sd = net.state_dict()
        with torch.no_grad():
            for name, a in _engine._unflatten(self._table, flat).items():
                t = torch.from_numpy(a)
                if sd[name].dim() == 3:
                    sd[name][:, :, sd[name].shape[2] // 2] = t
                else:
                    sd[name].copy_(t)

    def _attach(self):
        eng = self._engine()
        if eng._buffer is None:
            data = self._data
            if not isinstance(data, _engine.DeviceBuffer):
                obs, act = data
                buf = _engine.DeviceBuffer(self.obs_dim, self.act_dim, self._torch_device().index)
                z = np.zeros(len(obs), np.float32)
                buf.load(obs, act, obs, z, z)
                data = buf
            eng.attach_buffer(data)
        return eng

    # -- training ----------------------------------------------------------------------------
    def train(self):
        loaded = self.load_checkpoint(final=False)
        print(f"Loaded checkpoint. Starting from epoch {self.start_epoch}" if loaded else "No checkpoint found, starting from epoch 0")
        eng = self._attach()
        dev = self._torch_device()
        for epoch in range(self.start_epoch, int(self.c.num_epochs)):
            order = torch.randperm(self._n, device=dev)           # DataLoader(shuffle=True): one permutation, the last batch short
            for loss in eng.learn_epoch(order):
                self.logger.record_mean("train/loss", float(loss))
            self.logger.record("train/epoch", epoch, exclude=["tensorboard"])
            self.logger.dump(step=epoch)
            if (epoch + 1) % int(self.c.save_ckpt_freq) == 0:
                print(f"Saving checkpoint of epoch {epoch}")
                self.save_checkpoint(epoch=epoch)
        self._sync_from_engine()

    def _sync_from_engine(self):
        """the trained and the EMA weights back into the torch modules (inference and the final checkpoint use the EMA)"""
        eng = self._engine()
        self.unpack(eng.get(eng.PARAMS), self.noise_pred_net)
        if self.ema_noise_pred_net is None or self.ema_noise_pred_net is self.noise_pred_net:
            self.ema_noise_pred_net = copy.deepcopy(self.noise_pred_net)
        self.unpack(eng.get(eng.EMA), self.ema_noise_pred_net)
        self._ema_sd = self.ema_noise_pred_net.state_dict()

    # -- sampling ----------------------------------------------------------------------------
    def sample_init_noise(self, batch: int = 1) -> torch.Tensor:
        return torch.randn((batch, 1, self.act_dim), device=self._torch_device())

    def select_action_device(self, obs: torch.Tensor, init_noise: Optional[torch.Tensor] = None,
                             noise_index: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``obs`` [B, obs_dim] and ``init_noise`` [B, 1, act_dim] on the device -> actions [B, act_dim] on the device: N forward
        passes on the EMA weights and the DDPM updates between them, no host round trip.  With ``noise_index`` (int64 [B] on the
        device) ``init_noise`` is a table [n, 1, act_dim] and row i starts from ``init_noise[noise_index[i]]``, gathered by the
        sampler's first launch (the per-trajectory noise of ``rollout_device`` with the live trajectory indices)."""
        eng = self._engine()
        dev = self._torch_device()
        o = torch.as_tensor(obs, dtype=torch.float32, device=dev).reshape(-1, self.obs_dim).contiguous()
        if init_noise is None:
            init_noise = self.sample_init_noise(int(o.shape[0]))
        x = torch.as_tensor(init_noise, dtype=torch.float32, device=dev).reshape(-1, self.act_dim).contiguous()
        if noise_index is not None:
            idx = torch.as_tensor(noise_index, dtype=torch.int64, device=dev).contiguous()
            if idx.shape != (o.shape[0],):
                raise ValueError(f"select_action: {o.shape[0]} observations, noise_index of shape {tuple(idx.shape)}")
            return eng.sample(o, x, noise_idx=idx)
        if x.shape[0] != o.shape[0]:
            raise ValueError(f"select_action: {o.shape[0]} observations, {x.shape[0]} rows of init_noise")
        return eng.sample(o, x)

    def select_action(self, obs: np.ndarray, init_noise=None) -> np.ndarray:
        """obs (obs_dim) or (B, obs_dim); init_noise (B, 1, act_dim) from ``sample_init_noise`` -> (act_dim) or (B, act_dim)"""
        obs = np.asarray(obs, dtype=np.float32)
        act = self.select_action_device(torch.from_numpy(obs), init_noise).cpu().numpy()
        return act if obs.ndim == 2 else act[0]

    # -- checkpoints -------------------------------------------------------------------------
    def save_checkpoint(self, epoch: Optional[int]):
        """epoch None: the final model (``models.pt``, the EMA weights); else ``checkpoint.pt`` (the trained weights)"""
        final = epoch is None
        if self._eng is not None:
            self._sync_from_engine()
        if final:
            epoch = int(self.c.num_epochs) - 1
            if self.ema_noise_pred_net is None:
                raise RuntimeError("save_checkpoint(None): no EMA weights yet (train() or load_checkpoint(final=True) first)")
            sd = self.ema_noise_pred_net.state_dict()
        else:
            sd = self.noise_pred_net.state_dict()
        torch.save({"epoch": epoch, "model_state_dict": sd}, os.path.join(self.logger.dir, "models.pt" if final else "checkpoint.pt"))

    def load_checkpoint(self, final: bool = False) -> bool:
        if getattr(self.c, "path", None) is None:
            return False
        ckpt_path = os.path.join(self.c.path, "models.pt" if final else "checkpoint.pt")
        if not os.path.exists(ckpt_path):
            return False
        checkpoint = torch.load(ckpt_path, map_location="cpu")
        self.start_epoch = checkpoint["epoch"] + 1
        self.noise_pred_net.load_state_dict(checkpoint["model_state_dict"])
        if final:                                         # as in the reference: the loaded net IS the inference net
            self.ema_noise_pred_net = self.noise_pred_net
            self._ema_sd = self.noise_pred_net.state_dict()
        if self._eng is not None:                         # a fresh optimizer, schedule position and EMA, like the reference's resume
            flat = self.pack(self.noise_pred_net.state_dict())
            zero = np.zeros_like(flat)
            for which, arr in ((self._eng.PARAMS, flat), (self._eng.EMA, flat), (self._eng.EXP_AVG, zero), (self._eng.EXP_AVG_SQ, zero)):
                self._eng.set(which, arr)
            self._eng.step_count = 0
        return True

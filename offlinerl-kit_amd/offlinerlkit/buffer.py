"""ReplayBuffer with the reference's API (offlinerlkit/buffer/buffer.py:7-115) whose ``sample`` gathers from an
HBM-resident SoA copy of the data with a HIP kernel (csrc/kernels.h k_gather) through the C ABI.

Host numpy arrays are kept (``add`` / ``add_batch`` / ``sample_all`` / ``load_dataset`` semantics are unchanged);
the device copy is (re)uploaded lazily when they change.  After ``reserve_device()`` the roles swap: an HBM ring of ``_max_size`` rows
is the store, ``add`` / ``add_batch`` append to it on the device (``orl_buffer_append``), model rollouts land in it without touching
the host (``policy.rollout_device``), and the numpy arrays are a mirror that ``sync_host()`` / ``sample_all()`` refresh.  ``sample`` draws its indices with
``np.random.randint(0, size, batch_size)`` exactly like the reference (:98), so for a given numpy seed the index
stream — and therefore every minibatch — is identical to the reference's.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _engine


class ReplayBuffer:
    def __init__(self, buffer_size: int, obs_shape: Tuple, obs_dtype: np.dtype, action_dim: int, action_dtype: np.dtype,
                 device: str = "cpu") -> None:
        self._max_size = buffer_size
        self.obs_shape = tuple(obs_shape)
        self.obs_dtype = obs_dtype
        self.action_dim = int(action_dim)
        self.action_dtype = action_dtype
        self._ptr = 0
        self._size = 0
        self.observations = np.zeros((self._max_size,) + self.obs_shape, dtype=obs_dtype)
        self.next_observations = np.zeros((self._max_size,) + self.obs_shape, dtype=obs_dtype)
        self.actions = np.zeros((self._max_size, self.action_dim), dtype=action_dtype)
        self.rewards = np.zeros((self._max_size, 1), dtype=np.float32)
        self.terminals = np.zeros((self._max_size, 1), dtype=np.float32)
        self.device = torch.device(device)
        self._dev: Optional[_engine.DeviceBuffer] = None
        self._dirty = True
        self._ring = False            # reserve_device(): the HBM ring is the store, the numpy arrays a mirror
        self._host_stale = False

    # ---- host-side mutation (buffer.py:34-86) ----
    def add(self, obs, next_obs, action, reward, terminal) -> None:
        if self._ring:
            od = int(np.prod(self.obs_shape))
            return self.add_batch(np.asarray(obs).reshape(1, od), np.asarray(next_obs).reshape(1, od), np.asarray(action).reshape(1, -1),
                                  np.asarray(reward).reshape(1, 1), np.asarray(terminal).reshape(1, 1))
        self.observations[self._ptr] = np.array(obs).copy()
        self.next_observations[self._ptr] = np.array(next_obs).copy()
        self.actions[self._ptr] = np.array(action).copy()
        self.rewards[self._ptr] = np.array(reward).copy()
        self.terminals[self._ptr] = np.array(terminal).copy()
        self._ptr = (self._ptr + 1) % self._max_size
        self._size = min(self._size + 1, self._max_size)
        self._dirty = True

    def add_batch(self, obss, next_obss, actions, rewards, terminals) -> None:
        n = len(obss)
        if self._ring:
            od = int(np.prod(self.obs_shape))
            if torch.is_tensor(obss):
                self._dev.append(obss.reshape(n, od), actions, next_obss.reshape(n, od), rewards, terminals)
            else:
                self._dev.append(np.asarray(obss, np.float32).reshape(n, od), np.asarray(actions, np.float32),
                                 np.asarray(next_obss, np.float32).reshape(n, od), np.asarray(rewards, np.float32),
                                 np.asarray(terminals, np.float32))
            self._advance(n)
            return
        where = np.arange(self._ptr, self._ptr + n) % self._max_size
        self.observations[where] = np.array(obss).copy()
        self.next_observations[where] = np.array(next_obss).copy()
        self.actions[where] = np.array(actions).copy()
        self.rewards[where] = np.array(rewards).copy()
        self.terminals[where] = np.array(terminals).copy()
        self._ptr = (self._ptr + n) % self._max_size
        self._size = min(self._size + n, self._max_size)
        self._dirty = True

    def _advance(self, n: int) -> None:
        """host bookkeeping of ``n`` rows appended to the ring on the device (add_batch's, buffer.py:68-69)"""
        self._ptr = (self._ptr + n) % self._max_size
        self._size = min(self._size + n, self._max_size)
        self._host_stale = True

    def load_dataset(self, dataset: Dict[str, np.ndarray]) -> None:
        if self._ring:
            raise RuntimeError("load_dataset on a buffer whose store is the device ring (reserve_device): use add_batch")
        self.observations = np.array(dataset["observations"], dtype=self.obs_dtype)
        self.next_observations = np.array(dataset["next_observations"], dtype=self.obs_dtype)
        self.actions = np.array(dataset["actions"], dtype=self.action_dtype)
        self.rewards = np.array(dataset["rewards"], dtype=np.float32).reshape(-1, 1)
        self.terminals = np.array(dataset["terminals"], dtype=np.float32).reshape(-1, 1)
        self._ptr = len(self.observations)
        self._size = len(self.observations)
        self._dirty = True

    def normalize_obs(self, eps: float = 1e-3) -> Tuple[np.ndarray, np.ndarray]:
        """(x - mean) / (std + eps) on observations and next_observations (buffer.py:88-94).  The returned
        statistics are numpy's (what the reference returns); a resident device copy is normalised in place by the
        HIP kernel instead of being uploaded a second time."""
        if self._ring:
            raise RuntimeError("normalize_obs on a buffer whose store is the device ring (reserve_device) is not supported")
        mean = self.observations.mean(0, keepdims=True)
        std = self.observations.std(0, keepdims=True) + eps
        resident = self._dev is not None and not self._dirty and self._size == len(self.observations)
        self.observations = (self.observations - mean) / std
        self.next_observations = (self.next_observations - mean) / std
        if resident:
            self._dev.normalize_obs(eps)
        else:
            self._dirty = True
        return mean, std

    # ---- device side ----
    def _device_index(self) -> int:
        if self.device.type != "cuda":
            raise RuntimeError("offlinerlkit(AMD) ReplayBuffer.sample needs device='cuda' (the store lives in MI355X HBM; there is no CPU path)")
        return self.device.index if self.device.index is not None else torch.cuda.current_device()

    def reserve_device(self) -> "_engine.DeviceBuffer":
        """From now on the store is an HBM ring of ``_max_size`` rows (``orl_buffer_reserve``): ``add`` / ``add_batch`` append to it
        on the device, ``_ptr`` / ``_size`` stay correct on the host, ``sample`` gathers from it, ``sample_all`` and ``sync_host``
        refresh the numpy arrays from it.  Rows already in the buffer are carried over.  Idempotent."""
        if self._ring:
            return self._dev
        if self.observations.dtype != np.float32 or self.actions.dtype != np.float32:
            raise NotImplementedError("reserve_device: the device ring stores float32 observations and actions")
        od = int(np.prod(self.obs_shape))
        n, ptr = self._size, self._ptr
        if n and (len(self.observations) != self._max_size or ptr != n % self._max_size):
            # (the ring's write position follows from the rows appended to it: a wrapped host buffer cannot be carried over)
            raise NotImplementedError("reserve_device: call it before the host buffer wraps (and not on a loaded dataset)")
        if self._dev is None:
            self._dev = _engine.DeviceBuffer(od, self.action_dim, self._device_index())
        self._dev.reserve(self._max_size)
        self._ring = True
        if n:
            self._ptr, self._size = 0, 0
            self._dev.append(self.observations[:n].reshape(n, od), self.actions[:n], self.next_observations[:n].reshape(n, od),
                             self.rewards[:n], self.terminals[:n])
            self._advance(n)
            self._host_stale = False
        self._dirty = False
        return self._dev

    def sync_host(self) -> None:
        """refresh the numpy arrays from the device ring (``orl_buffer_read``); nothing to do for a host-backed buffer"""
        if not self._ring or not self._host_stale:
            return
        obs, act, nobs, rew, term = self._dev.read_rows(0, self._max_size)
        self.observations[...] = obs.reshape((self._max_size,) + self.obs_shape)
        self.next_observations[...] = nobs.reshape((self._max_size,) + self.obs_shape)
        self.actions[...] = act
        self.rewards[...] = rew
        self.terminals[...] = term
        self._host_stale = False

    def device_buffer(self) -> "_engine.DeviceBuffer":
        """The HBM-resident store (uploaded on first use / after host-side changes)."""
        if self._ring:
            return self._dev
        if self._size == 0:
            raise RuntimeError("ReplayBuffer is empty")
        if self._dev is None or self._dirty:
            od = int(np.prod(self.obs_shape))
            if self._dev is None:
                self._dev = _engine.DeviceBuffer(od, self.action_dim, self._device_index())
            n = self._size
            self._dev.load(self.observations[:n].reshape(n, od), self.actions[:n], self.next_observations[:n].reshape(n, od),
                           self.rewards[:n], self.terminals[:n])
            self._dirty = False
        return self._dev

    def sample(self, batch_size: int) -> Dict[str, torch.Tensor]:
        if self._ring and self._size == 0:
            raise RuntimeError("ReplayBuffer is empty")
        dev = self.device_buffer()
        batch_indexes = np.random.randint(0, self._size, size=batch_size)      # buffer.py:98
        od = int(np.prod(self.obs_shape))
        tdev = torch.device("cuda", self._device_index())
        out = {
            "observations": torch.empty((batch_size, od), dtype=torch.float32, device=tdev),
            "actions": torch.empty((batch_size, self.action_dim), dtype=torch.float32, device=tdev),
            "next_observations": torch.empty((batch_size, od), dtype=torch.float32, device=tdev),
            "terminals": torch.empty((batch_size, 1), dtype=torch.float32, device=tdev),
            "rewards": torch.empty((batch_size, 1), dtype=torch.float32, device=tdev),
        }
        torch.cuda.current_stream(tdev).synchronize()       # outputs are written on the null stream by the engine
        dev.sample_into(batch_indexes, batch_size, 0, out["observations"].data_ptr(), out["actions"].data_ptr(),
                        out["next_observations"].data_ptr(), out["rewards"].data_ptr(), out["terminals"].data_ptr())
        if len(self.obs_shape) != 1:
            out["observations"] = out["observations"].view((batch_size,) + self.obs_shape)
            out["next_observations"] = out["next_observations"].view((batch_size,) + self.obs_shape)
        return out

    def sample_all(self) -> Dict[str, np.ndarray]:
        self.sync_host()
        n = self._size
        return {
            "observations": self.observations[:n].copy(),
            "actions": self.actions[:n].copy(),
            "next_observations": self.next_observations[:n].copy(),
            "terminals": self.terminals[:n].copy(),
            "rewards": self.rewards[:n].copy(),
        }

"""MFPolicyTrainer (reference: offlinerlkit/policy_trainer/mf_policy_trainer.py:17-118) and MBPolicyTrainer (reference:
offlinerlkit/policy_trainer/mb_policy_trainer.py:17-198).

Same constructor, same logged keys, same per-epoch order (train steps -> lr_scheduler.step -> evaluate -> log ->
checkpoint) and the same return value.  Two inner loops:
  * ``fused=False``: the reference's loop verbatim — ``buffer.sample`` (numpy index stream) -> ``policy.learn``
    -> ``logger.logkv_mean`` per step, one host sync per step;
  * ``fused=True`` (default when the policy offers ``learn_n`` and the buffer is HBM-resident): the whole epoch's
    sample -> learn chain runs on the device and only the epoch means come back — the values ``logkv_mean`` would
    have accumulated (only per-epoch means are ever consumed).
Evaluation: ``eval_env`` may be ONE env (the reference's sequential loop, verbatim) or a list of envs, which are stepped in
lockstep with one batched ``select_action`` forward per step under the same episode accounting.
Several runs per policy object (``policy.n_runs`` > 1, BASELINE config 5): the epoch's training is still one ``learn_n``; every
run is evaluated, logged as ``run<i>/<key>`` (plain keys = mean over runs) and checkpointed as ``policy_run<i>.pth``.  With
``eval_env`` = one list of envs per run the runs are evaluated TOGETHER (one run-batched forward per env step,
``policy.select_action_runs``); with a single env or a flat list they are evaluated one after another (``select_run``).
Multi-GPU: independent runs, one process per GPU (replicas only).  When ``torch.distributed`` is initialised the
per-epoch metric vector of every rank is all-gathered (RCCL over xGMI on GPUs, gloo on CPU) so rank 0 can log
all runs; no other collective exists on this path.

MBPolicyTrainer is the reference's model-based loop (MOPO / COMBO): per step, a rollout every ``rollout_freq`` timesteps
(``policy.rollout`` from a ``real_buffer.sample`` of initial states, appended to ``fake_buffer``), then a real and a model minibatch
split by ``real_ratio`` and one ``policy.learn({"real": ..., "fake": ...})``.  The draw order, logged keys, checkpoints and the final
``dynamics.save`` are the reference's; evaluation, the multi-run ``run<i>/...`` keys and the per-run checkpoints are MFPolicyTrainer's.
``MBPolicyTrainer(fused=True)`` keeps the model buffer in an HBM ring and runs an epoch as device rollouts at the reference's
timesteps with ONE ``policy.learn_n`` between two of them (``fused_mb_schedule``); with ``dynamics_update_freq > 0`` (RAMBO) the chunks
are also cut at the model-update points (``fused_mb_dyn_schedule``) and ``policy.update_dynamics_device`` runs there.

RcslPolicyTrainer (reference: offlinerlkit/policy_trainer/rcsl_policy_trainer.py:21-365) is at the end of the module: one shuffled pass
over the dataset per epoch, in-process batches (``fused=False``) or one ``policy.learn_epoch`` on the device (``fused=True``).
"""
from __future__ import annotations

import os
import time
from collections import deque
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch


class MFPolicyTrainer:
    def __init__(self, policy, eval_env, buffer, logger, epoch: int = 1000, step_per_epoch: int = 1000, batch_size: int = 256,
                 eval_episodes: int = 10, lr_scheduler=None, fused: Optional[bool] = None, progress: bool = False) -> None:
        self.policy = policy
        self.eval_env = eval_env
        self.buffer = buffer
        self.logger = logger
        self._epoch = epoch
        self._step_per_epoch = step_per_epoch
        self._batch_size = batch_size
        self._eval_episodes = eval_episodes
        self.lr_scheduler = lr_scheduler
        if fused is None:
            fused = hasattr(policy, "learn_n") and hasattr(buffer, "device_buffer")
        self._fused = fused
        self._progress = progress
        self.gathered_metrics: List[Dict[str, np.ndarray]] = []   # per epoch: key -> value of every rank

    # ---- inner loops -----------------------------------------------------------------------
    def _train_epoch(self, e: int) -> int:
        if self._fused:
            means = self.policy.learn_n(self._step_per_epoch, self.buffer, self._batch_size)
            for k, v in means.items():
                self.logger.logkv(k, v)
            self._check_health()
            return self._step_per_epoch
        it = range(self._step_per_epoch)
        if self._progress:
            from tqdm import tqdm
            it = tqdm(it, desc=f"Epoch #{e}/{self._epoch}")
        for _ in it:
            batch = self.buffer.sample(self._batch_size)
            loss = self.policy.learn(batch)
            if self._progress:
                it.set_postfix(**loss)
            for k, v in loss.items():
                self.logger.logkv_mean(k, v)
        self._check_health()
        return self._step_per_epoch

    def _check_health(self) -> None:
        """once per epoch: the engine's range / non-finite scan (EnginePolicy.check_health warns or raises); other policies have none"""
        check = getattr(self.policy, "check_health", None)
        if callable(check):
            check()

    def _gather(self, kv: Dict[str, float]) -> None:
        """End-of-epoch metric all-gather: every rank contributes its metric vector, rank 0 logs ``rank<i>/<key>``."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        keys = sorted(kv)
        backend = dist.get_backend()
        dev = torch.device("cuda", torch.cuda.current_device()) if backend == "nccl" else torch.device("cpu")
        mine = torch.tensor([float(kv[k]) for k in keys], dtype=torch.float32, device=dev)
        out = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
        dist.all_gather(out, mine)
        table = torch.stack(out).cpu().numpy()
        self.gathered_metrics.append({k: table[:, i].copy() for i, k in enumerate(keys)})
        if dist.get_rank() == 0:
            for r in range(table.shape[0]):
                for i, k in enumerate(keys):
                    self.logger.logkv(f"rank{r}/{k}", float(table[r, i]))

    # ---- reference API ---------------------------------------------------------------------
    def train(self) -> Dict[str, float]:
        start_time = time.time()
        num_timesteps = 0
        last_10_performance = deque(maxlen=10)
        n_runs = int(getattr(self.policy, "n_runs", 1))
        for e in range(1, self._epoch + 1):
            self.policy.train()
            num_timesteps += self._train_epoch(e)
            if self.lr_scheduler is not None:
                self.lr_scheduler.step()
            if n_runs == 1:
                eval_info = self._evaluate()
            else:
                grouped = self._env_groups(n_runs)
                per_run_all = self._evaluate_runs_batched(grouped) if grouped is not None else None
                per_run = []
                for r in range(n_runs):
                    if per_run_all is not None:
                        per_run.append(per_run_all[r])
                    else:
                        self.policy.select_run(r)
                        per_run.append(self._evaluate())
                    self.logger.logkv(f"run{r}/eval/episode_reward", float(np.mean(per_run[-1]["eval/episode_reward"])))
                    self.logger.logkv(f"run{r}/eval/episode_length", float(np.mean(per_run[-1]["eval/episode_length"])))
                    if hasattr(self._score_env(), "get_normalized_score"):
                        self.logger.logkv(f"run{r}/eval/normalized_episode_reward",
                                          self._score_env().get_normalized_score(float(np.mean(per_run[-1]["eval/episode_reward"]))) * 100)
                self.policy.select_run(0)
                eval_info = {k: [x for info in per_run for x in info[k]] for k in per_run[0]}      # pooled over runs
            ep_reward_mean, ep_reward_std = np.mean(eval_info["eval/episode_reward"]), np.std(eval_info["eval/episode_reward"])
            ep_length_mean, ep_length_std = np.mean(eval_info["eval/episode_length"]), np.std(eval_info["eval/episode_length"])
            epoch_kv = dict(self.logger._name2val) if hasattr(self.logger, "_name2val") else {}
            if hasattr(self._score_env(), "get_normalized_score"):
                norm_ep_rew_mean = self._score_env().get_normalized_score(ep_reward_mean) * 100
                norm_ep_rew_std = self._score_env().get_normalized_score(ep_reward_std) * 100
                last_10_performance.append(norm_ep_rew_mean)
                self.logger.logkv("eval/normalized_episode_reward", norm_ep_rew_mean)
                self.logger.logkv("eval/normalized_episode_reward_std", norm_ep_rew_std)
                epoch_kv["eval/normalized_episode_reward"] = norm_ep_rew_mean
            self.logger.logkv("eval/episode_reward", ep_reward_mean)
            self.logger.logkv("eval/episode_reward_std", ep_reward_std)
            self.logger.logkv("eval/episode_length", ep_length_mean)
            self.logger.logkv("eval/episode_length_std", ep_length_std)
            epoch_kv["eval/episode_reward"] = ep_reward_mean
            self._gather({k: v for k, v in epoch_kv.items() if isinstance(v, (int, float, np.floating))})
            self.logger.set_timestep(num_timesteps)
            self.logger.dumpkvs()
            self._checkpoint(self.logger.checkpoint_dir, n_runs)
        self.logger.log("total time: {:.2f}s".format(time.time() - start_time))
        self._checkpoint(self.logger.model_dir, n_runs)
        self.logger.close()
        return {"last_10_performance": np.mean(last_10_performance)}

    def _checkpoint(self, where: str, n_runs: int) -> None:
        torch.save(self.policy.state_dict(), os.path.join(where, "policy.pth"))          # (run 0 when the policy carries several)
        if n_runs > 1:
            for r in range(n_runs):
                torch.save(self.policy.run_state_dict(r), os.path.join(where, f"policy_run{r}.pth"))

    def _score_env(self):
        e = self.eval_env
        while isinstance(e, (list, tuple)):
            e = e[0]
        return e

    def _evaluate(self) -> Dict[str, List[float]]:
        if isinstance(self.eval_env, (list, tuple)):
            return self._evaluate_batched(list(self.eval_env))
        self.policy.eval()
        obs = self.eval_env.reset()
        done_eps: List[Dict[str, float]] = []
        ep_reward, ep_len = 0, 0
        while len(done_eps) < self._eval_episodes:
            action = self.policy.select_action(obs.reshape(1, -1), deterministic=True)
            obs, reward, terminal, _ = self.eval_env.step(action.flatten())
            ep_reward += reward
            ep_len += 1
            if terminal:
                done_eps.append({"episode_reward": ep_reward, "episode_length": ep_len})
                ep_reward, ep_len = 0, 0
                obs = self.eval_env.reset()
        return {"eval/episode_reward": [d["episode_reward"] for d in done_eps],
                "eval/episode_length": [d["episode_length"] for d in done_eps]}

    def _env_groups(self, n_runs: int):
        """``eval_env`` given as one list of envs PER RUN ([[env, ...]] * n_runs) -> those groups, else None (sequential evaluation)"""
        ev = self.eval_env
        if isinstance(ev, (list, tuple)) and len(ev) == n_runs and all(isinstance(g, (list, tuple)) and len(g) > 0 for g in ev) \
                and len({len(g) for g in ev}) == 1 and hasattr(self.policy, "select_action_runs"):
            return [list(g) for g in ev]
        return None

    def _evaluate_runs_batched(self, groups) -> List[Dict[str, List[float]]]:
        """All runs of a multi-run policy evaluated together: run r owns the envs ``groups[r]``; every step is ONE run-batched
        deterministic forward over [n_runs, E, obs_dim] (``policy.select_action_runs``) instead of n_runs x E one-row forwards and
        n_runs full rollouts one after another.  Per run the episode accounting is ``_evaluate_batched``'s."""
        self.policy.eval()
        R, E = len(groups), len(groups[0])
        obs = [[np.asarray(env.reset(), dtype=np.float32).reshape(-1) for env in g] for g in groups]
        started = [min(E, self._eval_episodes)] * R
        active = [[i < started[r] for i in range(E)] for r in range(R)]
        ep_reward = [[0.0] * E for _ in range(R)]
        ep_len = [[0] * E for _ in range(R)]
        done_eps: List[List[Dict[str, float]]] = [[] for _ in range(R)]
        while any(len(d) < self._eval_episodes for d in done_eps):
            actions = self.policy.select_action_runs(np.stack([np.stack(o) for o in obs]))
            for r in range(R):
                for i in range(E):
                    if not active[r][i]:
                        continue
                    o, reward, terminal, _ = groups[r][i].step(np.asarray(actions[r, i]).flatten())
                    obs[r][i] = np.asarray(o, dtype=np.float32).reshape(-1)
                    ep_reward[r][i] += reward
                    ep_len[r][i] += 1
                    if terminal:
                        done_eps[r].append({"episode_reward": ep_reward[r][i], "episode_length": ep_len[r][i]})
                        ep_reward[r][i], ep_len[r][i] = 0.0, 0
                        if started[r] < self._eval_episodes:
                            started[r] += 1
                            obs[r][i] = np.asarray(groups[r][i].reset(), dtype=np.float32).reshape(-1)
                        else:
                            active[r][i] = False
        return [{"eval/episode_reward": [d["episode_reward"] for d in de], "eval/episode_length": [d["episode_length"] for d in de]}
                for de in done_eps]

    def _evaluate_batched(self, envs) -> Dict[str, List[float]]:
        """E envs in lockstep: one [E, obs_dim] deterministic forward per step instead of E one-row forwards.  Episode accounting
        as in the reference loop: an env that finishes an episode is reset and keeps running while episodes are still owed; the
        first ``eval_episodes`` episodes to START are the ones reported, in order of completion."""
        self.policy.eval()
        E = len(envs)
        obs = [env.reset() for env in envs]
        started = min(E, self._eval_episodes)
        active = [i < started for i in range(E)]
        ep_reward, ep_len = [0.0] * E, [0] * E
        done_eps: List[Dict[str, float]] = []
        while len(done_eps) < self._eval_episodes:
            idx = [i for i in range(E) if active[i]]
            batch = np.stack([np.asarray(obs[i], dtype=np.float32).reshape(-1) for i in idx])
            actions = self.policy.select_action(batch, deterministic=True)
            for j, i in enumerate(idx):
                o, reward, terminal, _ = envs[i].step(np.asarray(actions[j]).flatten())
                obs[i] = o
                ep_reward[i] += reward
                ep_len[i] += 1
                if terminal:
                    done_eps.append({"episode_reward": ep_reward[i], "episode_length": ep_len[i]})
                    ep_reward[i], ep_len[i] = 0.0, 0
                    if started < self._eval_episodes:
                        started += 1
                        obs[i] = envs[i].reset()
                    else:
                        active[i] = False
        return {"eval/episode_reward": [d["episode_reward"] for d in done_eps],
                "eval/episode_length": [d["episode_length"] for d in done_eps]}


def _host(x) -> np.ndarray:
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def fused_mb_schedule(num_timesteps: int, step_per_epoch: int, rollout_freq: int) -> List[Tuple[bool, int]]:
    """One epoch of the model-based loop (mb_policy_trainer.py:66-102) that starts at timestep ``num_timesteps``, as chunks
    ``(rollout_first, n_steps)``: a rollout happens in front of exactly the timesteps ``t`` with ``t % rollout_freq == 0``, and the
    training steps between two such points (or up to the epoch's end) form one chunk.  No chunk is empty and the lengths sum to
    ``step_per_epoch``."""
    if rollout_freq < 1 or step_per_epoch < 0:
        raise ValueError("rollout_freq must be >= 1 and step_per_epoch >= 0")
    out, t, end = [], num_timesteps, num_timesteps + step_per_epoch
    while t < end:
        nxt = min(end, (t // rollout_freq + 1) * rollout_freq)
        out.append((t % rollout_freq == 0, nxt - t))
        t = nxt
    return out


def fused_mb_dyn_schedule(num_timesteps: int, step_per_epoch: int, rollout_freq: int, dynamics_update_freq: int = 0
                          ) -> List[Tuple[bool, int, bool]]:
    """``fused_mb_schedule`` with RAMBO's model updates (mb_policy_trainer.py:95-99): chunks ``(rollout_first, n_steps,
    update_dynamics_after)``, cut at the rollout points AND behind every timestep ``t`` with ``(t + 1) % dynamics_update_freq == 0``,
    where the model update runs after the chunk's training steps.  ``dynamics_update_freq`` 0: ``fused_mb_schedule``'s chunks, no update."""
    if dynamics_update_freq < 0:
        raise ValueError("dynamics_update_freq must be >= 0")
    out = []
    for rollout_first, steps in fused_mb_schedule(num_timesteps, step_per_epoch, rollout_freq):
        t, end = num_timesteps, num_timesteps + steps
        while t < end:
            nxt = min(end, (t // dynamics_update_freq + 1) * dynamics_update_freq) if dynamics_update_freq > 0 else end
            out.append((rollout_first and t == num_timesteps, nxt - t, dynamics_update_freq > 0 and nxt % dynamics_update_freq == 0))
            t = nxt
        num_timesteps = end
    return out


class MBPolicyTrainer(MFPolicyTrainer):
    """Constructor = mb_policy_trainer.py:18-55.  ``rollout_setting`` = (rollout_freq, rollout_batch_size, rollout_length).

    ``fused=True`` runs an epoch on the device: at every timestep ``t`` with ``t % rollout_freq == 0`` one ``policy.rollout_device``
    into ``fake_buffer``'s HBM ring (``fake_buffer.reserve_device()``, called here), and between those points ONE
    ``policy.learn_n(steps, real_buffer, fake_buffer, batch_size, real_ratio)``.  The logged loss keys are the step-weighted means of
    the chunks (what ``logkv_mean`` holds after the same steps); the rollout log line, the ``rollout_info/*`` keys, evaluation,
    checkpoints, health check and ``dynamics.save`` are those of the host loop.  ``fake_buffer`` may be a sequence of ``policy.n_runs``
    buffers: one model ring per run, run r rolled by its own actor through run r of the dynamics (or a shared one-run ensemble) and
    sampled by run r only; ``run<r>/rollout_info/*`` per run, the plain keys their mean (``fused=True`` only).  What differs from the host loop: the minibatch indices
    of both buffers come from the device Philox stream instead of numpy's (as for ``MFPolicyTrainer(fused=True)``), and the model
    draws of a rollout from the dynamics' device stream; runs are reproducible from the seed but not index-identical to the
    reference.  ``dynamics_update_freq > 0`` needs a policy with ``update_dynamics_device`` (RAMBO): the chunks are then also cut behind
    every timestep ``t`` with ``(t + 1) % dynamics_update_freq == 0`` (``fused_mb_dyn_schedule``), the model update runs there as one
    device loop and its five values go through ``logkv_mean`` as in the host loop.  Refused at construction:
    ``dynamics_update_freq > 0`` with any other policy (its dynamics has no device update), a policy without ``rollout_device``,
    a dynamics whose termination function is not one of the fixed row-wise tests (no ``term_kind``)."""

    def __init__(self, policy, eval_env, real_buffer, fake_buffer, logger, rollout_setting: Tuple[int, int, int], epoch: int = 1000,
                 step_per_epoch: int = 1000, batch_size: int = 256, real_ratio: float = 0.05, eval_episodes: int = 10,
                 lr_scheduler=None, dynamics_update_freq: int = 0, horizon: Optional[int] = None, progress: bool = False,
                 fused: bool = False) -> None:
        super().__init__(policy, eval_env, real_buffer, logger, epoch=epoch, step_per_epoch=step_per_epoch, batch_size=batch_size,
                         eval_episodes=eval_episodes, lr_scheduler=lr_scheduler, fused=False, progress=progress)
        self.real_buffer = real_buffer
        self.fake_buffer = fake_buffer
        self.horizon = horizon
        self._rollout_freq, self._rollout_batch_size, self._rollout_length = rollout_setting
        self._dynamics_update_freq = dynamics_update_freq
        self._real_ratio = real_ratio
        self.is_gymnasium_env = hasattr(self._score_env(), "get_true_observation")
        assert (not self.is_gymnasium_env) or (self.horizon is not None), "Horizon must be specified for Gymnasium env"
        self._fused_mb = bool(fused)
        if self._fused_mb:
            if dynamics_update_freq > 0 and not hasattr(policy, "update_dynamics_device"):
                raise ValueError("MBPolicyTrainer(fused=True): dynamics_update_freq > 0 is not supported (only RAMBO has update_dynamics, "
                                 "and its dynamics changes between the steps of a chunk)")
            if not (hasattr(policy, "rollout_device") and hasattr(policy, "learn_n")):
                raise ValueError(f"MBPolicyTrainer(fused=True): {type(policy).__name__} has no rollout_device / two-buffer learn_n")
            if getattr(getattr(policy, "dynamics", None), "term_kind", None) is None:
                raise ValueError("MBPolicyTrainer(fused=True): the dynamics' termination function is not one of the fixed row-wise tests of "
                                 "utils.termination_fns (no term_kind: an obs_unnormalization wrapper, door or another callable), so the "
                                 "device rollout cannot evaluate it; use fused=False")
        from .policy.model_based import per_run_rings
        self._fake_runs = per_run_rings(policy, fake_buffer)          # a sequence of n_runs buffers: one model ring per run
        if self._fake_runs is not None and not self._fused_mb:
            raise ValueError("MBPolicyTrainer(fused=False): per-run model buffers (a sequence as fake_buffer) need fused=True; the host "
                             "loop stays the reference's single-buffer loop")
        if self._fused_mb:
            if self._fake_runs is not None:
                dyn_runs = int(getattr(policy.dynamics, "_n_runs", 1))
                if dyn_runs not in (1, len(self._fake_runs)):
                    raise ValueError(f"MBPolicyTrainer(fused=True): per-run model buffers need a dynamics of {len(self._fake_runs)} runs "
                                     f"(run r rolls through ensemble r) or of one shared run, this one carries {dyn_runs}")
                for b in self._fake_runs:
                    b.reserve_device()
            else:
                fake_buffer.reserve_device()

    # ---- the reference's inner loop (mb_policy_trainer.py:66-102) -----------------------------------------
    def _rollout(self) -> None:
        init_obss = _host(self.real_buffer.sample(self._rollout_batch_size)["observations"])
        rollout_transitions, rollout_info = self.policy.rollout(init_obss, self._rollout_length)
        self.fake_buffer.add_batch(**rollout_transitions)
        self.logger.log("num rollout transitions: {}, reward mean: {:.4f}".format(rollout_info["num_transitions"], rollout_info["reward_mean"]))
        for k, v in rollout_info.items():
            self.logger.logkv_mean("rollout_info/" + k, v)

    def _rollout_fused(self) -> None:
        rollout_info = self.policy.rollout_device(self.real_buffer, self.fake_buffer, self._rollout_batch_size, self._rollout_length)
        if self._fake_runs is not None:
            # per-run rings: run<r>/rollout_info/* per run, the plain keys = mean over runs (as the loss keys); the log line carries the
            # summed transitions and the transition-weighted reward mean
            nt, rm = np.asarray(rollout_info["num_transitions"], np.float64), np.asarray(rollout_info["reward_mean"], np.float64)
            self.logger.log("num rollout transitions: {}, reward mean: {:.4f}".format(int(nt.sum()), float((nt * rm).sum() / max(nt.sum(), 1.0))))
            for r in range(len(nt)):
                self.logger.logkv_mean(f"run{r}/rollout_info/num_transitions", float(nt[r]))
                self.logger.logkv_mean(f"run{r}/rollout_info/reward_mean", float(rm[r]))
            self.logger.logkv_mean("rollout_info/num_transitions", float(nt.mean()))
            self.logger.logkv_mean("rollout_info/reward_mean", float(rm.mean()))
            return
        self.logger.log("num rollout transitions: {}, reward mean: {:.4f}".format(rollout_info["num_transitions"], rollout_info["reward_mean"]))
        for k, v in rollout_info.items():
            self.logger.logkv_mean("rollout_info/" + k, v)

    def _train_mb_epoch_fused(self, e: int, num_timesteps: int) -> int:
        sums: Dict[str, float] = {}
        for rollout_first, steps, update_after in fused_mb_dyn_schedule(num_timesteps, self._step_per_epoch, self._rollout_freq,
                                                                        self._dynamics_update_freq):
            if rollout_first:
                self._rollout_fused()
            means = self.policy.learn_n(steps, self.real_buffer, self.fake_buffer, self._batch_size, self._real_ratio)
            for k, v in means.items():
                sums[k] = sums.get(k, 0.0) + float(v) * steps
            num_timesteps += steps
            if update_after:      # RAMBO (mb_policy_trainer.py:95-99): the adversarial model update, one call into the device loop
                for k, v in self.policy.update_dynamics_device(self.real_buffer).items():
                    self.logger.logkv_mean(k, v)
        for k, v in sums.items():
            self.logger.logkv(k, v / self._step_per_epoch)
        self._check_health()
        return num_timesteps

    def _train_mb_epoch(self, e: int, num_timesteps: int) -> int:
        if self._fused_mb:
            return self._train_mb_epoch_fused(e, num_timesteps)
        it = range(self._step_per_epoch)
        if self._progress:
            from tqdm import tqdm
            it = tqdm(it, desc=f"Epoch #{e}/{self._epoch}")
        for _ in it:
            if num_timesteps % self._rollout_freq == 0:
                self._rollout()
            real_sample_size = int(self._batch_size * self._real_ratio)
            fake_sample_size = self._batch_size - real_sample_size
            real_batch = self.real_buffer.sample(batch_size=real_sample_size)
            fake_batch = self.fake_buffer.sample(batch_size=fake_sample_size)
            loss = self.policy.learn({"real": real_batch, "fake": fake_batch})
            if self._progress:
                it.set_postfix(**loss)
            for k, v in loss.items():
                self.logger.logkv_mean(k, v)
            if 0 < self._dynamics_update_freq and (num_timesteps + 1) % self._dynamics_update_freq == 0:
                for k, v in self.policy.update_dynamics(self.real_buffer).items():
                    self.logger.logkv_mean(k, v)
            num_timesteps += 1
        self._check_health()
        return num_timesteps

    # ---- reference API ---------------------------------------------------------------------
    def train(self) -> Dict[str, float]:
        start_time = time.time()
        num_timesteps = 0
        last_10_performance = deque(maxlen=10)
        n_runs = int(getattr(self.policy, "n_runs", 1))
        for e in range(1, self._epoch + 1):
            self.policy.train()
            num_timesteps = self._train_mb_epoch(e, num_timesteps)
            if self.lr_scheduler is not None:
                self.lr_scheduler.step()
            if n_runs == 1:
                eval_info = self._evaluate()
            else:
                grouped = self._env_groups(n_runs) if self.horizon is None and not self.is_gymnasium_env else None
                per_run_all = self._evaluate_runs_batched(grouped) if grouped is not None else None
                per_run = []
                for r in range(n_runs):
                    if per_run_all is not None:
                        per_run.append(per_run_all[r])
                    else:
                        self.policy.select_run(r)
                        per_run.append(self._evaluate())
                    self._log_eval(per_run[-1], f"run{r}/", None)
                self.policy.select_run(0)
                eval_info = {k: [x for info in per_run for x in info[k]] for k in per_run[0]}      # pooled over runs
            self._log_eval(eval_info, "", last_10_performance)
            self.logger.set_timestep(num_timesteps)
            self.logger.dumpkvs(exclude=["dynamics_training_progress"])
            self._checkpoint(self.logger.checkpoint_dir, n_runs)
        self.logger.log("total time: {:.2f}s".format(time.time() - start_time))
        self._checkpoint(self.logger.model_dir, n_runs)
        self.policy.dynamics.save(self.logger.model_dir)
        self.logger.close()
        return {"last_10_performance": np.mean(last_10_performance)}

    def _log_eval(self, eval_info: Dict[str, List[float]], prefix: str, last_10: Optional[deque]) -> None:
        """mb_policy_trainer.py:108-121: gymnasium envs log the raw return, the others the normalised one (never both)"""
        ep_reward_mean, ep_reward_std = np.mean(eval_info["eval/episode_reward"]), np.std(eval_info["eval/episode_reward"])
        ep_length_mean, ep_length_std = np.mean(eval_info["eval/episode_length"]), np.std(eval_info["eval/episode_length"])
        if self.is_gymnasium_env:
            if last_10 is not None:
                last_10.append(ep_reward_mean)
            self.logger.logkv(prefix + "eval/episode_reward", ep_reward_mean)
            self.logger.logkv(prefix + "eval/episode_reward_std", ep_reward_std)
        else:
            env = self._score_env()
            norm_ep_rew_mean = env.get_normalized_score(ep_reward_mean) * 100
            norm_ep_rew_std = env.get_normalized_score(ep_reward_std) * 100
            if last_10 is not None:
                last_10.append(norm_ep_rew_mean)
            self.logger.logkv(prefix + "eval/normalized_episode_reward", norm_ep_rew_mean)
            self.logger.logkv(prefix + "eval/normalized_episode_reward_std", norm_ep_rew_std)
        self.logger.logkv(prefix + "eval/episode_length", ep_length_mean)
        self.logger.logkv(prefix + "eval/episode_length_std", ep_length_std)

    def _evaluate(self) -> Dict[str, List[float]]:
        """mb_policy_trainer.py:131-198: a fixed ``horizon`` per episode (terminals ignored) and gymnasium envs on one env; without
        either, MFPolicyTrainer's evaluation (the same episode loop, or lockstep envs for a list)"""
        if self.horizon is None and not self.is_gymnasium_env:
            return super()._evaluate()
        env = self.eval_env
        gym_api = self.is_gymnasium_env
        self.policy.eval()

        def reset():
            if gym_api:
                o, _ = env.reset()
                return env.get_true_observation(o)
            return env.reset()

        def step(o):
            action = self.policy.select_action(o.reshape(1, -1), deterministic=True)
            if gym_api:
                nxt, reward, terminal, _, _ = env.step(action.flatten())
                return env.get_true_observation(nxt), reward, terminal
            nxt, reward, terminal, _ = env.step(action.flatten())
            return nxt, reward, terminal

        obs = reset()
        done_eps: List[Dict[str, float]] = []
        ep_reward, ep_len = 0, 0
        while len(done_eps) < self._eval_episodes:
            if self.horizon is not None:
                for _ in range(self.horizon):
                    obs, reward, _ = step(obs)
                    ep_reward += reward
                    ep_len += 1
                finished = True
            else:
                obs, reward, finished = step(obs)
                ep_reward += reward
                ep_len += 1
            if finished:
                done_eps.append({"episode_reward": ep_reward, "episode_length": ep_len})
                ep_reward, ep_len = 0, 0
                obs = reset()
        return {"eval/episode_reward": [d["episode_reward"] for d in done_eps],
                "eval/episode_length": [d["episode_length"] for d in done_eps]}


class DictDataset(torch.utils.data.Dataset):
    """A dict of equally long arrays as a map-style dataset: item i is ``{key: array[i]}`` (reference: utils/dataset.py DictDataset)."""

    def __init__(self, dataset: Dict[str, np.ndarray]) -> None:
        self._data = dict(dataset)
        self._len = len(next(iter(self._data.values())))

    def __len__(self) -> int:
        return self._len

    def __getitem__(self, idx):
        return {k: v[idx] for k, v in self._data.items()}


class RcslPolicyTrainer:
    """RcslPolicyTrainer (reference: offlinerlkit/policy_trainer/rcsl_policy_trainer.py:21-365): per epoch ONE pass over the shuffled
    dataset -- every row once, last batch partial --, ``lr_scheduler.step()``, evaluation conditioned on ``goal`` (the return-to-go starts at
    ``goal`` and drops by every reward), the reference's logged keys in its order, ``checkpoint_dir/policy.pth`` each epoch and
    ``model_dir/policy.pth`` at the end.  ``offline_ratio`` 0 trains on ``rollout_dataset``, 1 on ``offline_dataset``; anything else is refused.

    ``rollout_dataset`` may also be the dict of ``rollout()`` / ``DeviceRollout.to_host()`` (``obss`` / ``next_obss`` keys) or, on the
    fused path, a ``DeviceBuffer`` that already holds returns-to-go in its reward column (``DeviceRollout.export``,
    ``collect_rollouts_device``): it is trained on as it is, nothing is uploaded.

    ``fused=False``: the batches of a shuffled ``DataLoader`` drawn in this process (``num_workers`` is accepted and ignored: no worker
    process is ever started), each through ``policy.learn``.  ``fused=True`` (the default when the policy has ``learn_epoch`` and a GPU is
    visible): the dataset is loaded once into a ``DeviceBuffer`` with ``rtgs`` in its reward column, and an epoch is one ``torch.randperm``
    per run, padded with -1 to a multiple of the batch size, and one ``policy.learn_epoch``."""

    def __init__(self, policy, eval_env, offline_dataset: Dict[str, np.ndarray], rollout_dataset: Dict[str, np.ndarray], goal: float, logger,
                 seed, eval_env2=None, epoch: int = 1000, step_per_epoch: int = 1000, batch_size: int = 256, offline_ratio: float = 0,
                 eval_episodes: int = 10, lr_scheduler=None, horizon: Optional[int] = None, num_workers=1,
                 fused: Optional[bool] = None) -> None:
        self.policy = policy
        self.eval_env = eval_env
        self.eval_env2 = eval_env2
        self.horizon = horizon
        self.offline_dataset = offline_dataset
        self.rollout_dataset = rollout_dataset
        self.goal = goal
        self.logger = logger
        self._epoch = epoch
        self._step_per_epoch = step_per_epoch
        self._batch_size = batch_size
        self._offline_ratio = offline_ratio
        self._eval_episodes = eval_episodes
        self.lr_scheduler = lr_scheduler
        self.num_workers = num_workers
        self.env_seed = seed
        self.is_gymnasium_env = hasattr(self.eval_env, "get_true_observation")
        assert (not self.is_gymnasium_env) or (self.horizon is not None), "Horizon must be specified for Gymnasium env"
        if fused is None:
            fused = hasattr(policy, "learn_epoch") and torch.cuda.is_available()
        self._fused = bool(fused)
        self._dbuf = None

    def _dataset(self) -> Dict[str, np.ndarray]:
        if self._offline_ratio == 0:
            return self.rollout_dataset
        if self._offline_ratio == 1:
            return self.offline_dataset
        raise NotImplementedError

    def _device_buffer(self, data):
        """the training data as a ``DeviceBuffer`` with rtgs in its reward column: a ``DeviceBuffer`` that already is one (an exported
        device rollout) as it is; a dict with ``observations`` / ``next_observations``, or with the ``obss`` / ``next_obss`` of
        ``rollout()`` (the two spellings the reference's ``DictDataset`` serves), uploaded once"""
        from . import _engine
        if isinstance(data, _engine.DeviceBuffer):
            if data.size() < 1:
                raise ValueError("RcslPolicyTrainer: the rollout DeviceBuffer is empty")
            return data
        ko, kn = ("observations", "next_observations") if "observations" in data else ("obss", "next_obss")
        obs = np.asarray(data[ko], dtype=np.float32)
        act = np.asarray(data["actions"], dtype=np.float32)
        n = len(obs)
        nxt = np.asarray(data[kn], dtype=np.float32) if kn in data else obs
        term = np.asarray(data["terminals"], dtype=np.float32).reshape(n) if "terminals" in data else np.zeros(n, np.float32)
        dev = torch.cuda.current_device()
        pdev = getattr(getattr(self.policy, "rcsl", None), "device", None)
        if pdev is not None and torch.device(pdev).type == "cuda" and torch.device(pdev).index is not None:
            dev = torch.device(pdev).index
        buf = _engine.DeviceBuffer(obs.shape[1], act.shape[1], dev)
        buf.load(obs, act, nxt, np.asarray(data["rtgs"], dtype=np.float32).reshape(n), term)      # rtgs travel in the reward column
        return buf

    def _train_epoch(self, data: Dict[str, np.ndarray], loader) -> int:
        from .policy.rcsl import epoch_order
        if self._fused:
            order = epoch_order(self._dbuf.size(), self._batch_size, int(getattr(self.policy, "n_runs", 1)))
            means = self.policy.learn_epoch(self._dbuf, order, self._batch_size)
            for k, v in means.items():
                self.logger.logkv(k, v)
            return order.shape[1] // self._batch_size
        steps = 0
        for batch in loader:
            loss_dict = self.policy.learn(batch)
            for k, v in loss_dict.items():
                self.logger.logkv_mean(k, v)
            steps += 1
        return steps

    def train(self) -> Dict[str, float]:
        start_time = time.time()
        num_timesteps = 0
        last_10_performance = deque(maxlen=10)
        data = self._dataset()
        loader = None
        if self._fused:
            self._dbuf = self._device_buffer(data)
        elif not isinstance(data, dict):
            raise NotImplementedError("RcslPolicyTrainer(fused=False) trains on a dict of host arrays; a DeviceBuffer needs fused=True")
        else:
            # the reference's DataLoader(shuffle=True) with the batches collated in THIS process: num_workers = 0 whatever was asked for
            loader = torch.utils.data.DataLoader(DictDataset(data), batch_size=self._batch_size, shuffle=True, num_workers=0)
        for e in range(1, self._epoch + 1):
            self.policy.train()
            num_timesteps += self._train_epoch(data, loader)
            if self.lr_scheduler is not None:
                self.lr_scheduler.step()
            check = getattr(self.policy, "check_health", None)
            if callable(check):
                check()
            eval_info = self._evaluate()
            ep_reward_mean, ep_reward_std = np.mean(eval_info["eval/episode_reward"]), np.std(eval_info["eval/episode_reward"])
            ep_reward_max, ep_reward_min = np.max(eval_info["eval/episode_reward"]), np.min(eval_info["eval/episode_reward"])
            ep_length_mean, ep_length_std = np.mean(eval_info["eval/episode_length"]), np.std(eval_info["eval/episode_length"])
            normalized = hasattr(self.eval_env, "get_normalized_score")
            if not normalized:
                last_10_performance.append(ep_reward_mean)
                self.logger.logkv("eval/episode_reward", ep_reward_mean)
                self.logger.logkv("eval/episode_reward_std", ep_reward_std)
            else:
                norm_ep_rew_mean = self.eval_env.get_normalized_score(ep_reward_mean) * 100
                last_10_performance.append(norm_ep_rew_mean)
                self.logger.logkv("eval/normalized_episode_reward", norm_ep_rew_mean)
                self.logger.logkv("eval/normalized_episode_reward_std", self.eval_env.get_normalized_score(ep_reward_std) * 100)
                self.logger.logkv("eval/normalized_episode_reward_max", self.eval_env.get_normalized_score(ep_reward_max) * 100)
                self.logger.logkv("eval/normalized_episode_reward_min", self.eval_env.get_normalized_score(ep_reward_min) * 100)
            self.logger.logkv("eval/episode_length", ep_length_mean)
            self.logger.logkv("eval/episode_length_std", ep_length_std)
            if self.eval_env2 is not None:
                info2 = self._evaluate_no_fix_seed()
                rew2_mean, rew2_std = np.mean(info2["eval/episode_reward"]), np.std(info2["eval/episode_reward"])
                len2_mean, len2_std = np.mean(info2["eval/episode_length"]), np.std(info2["eval/episode_length"])
                # (the reference appends the FIXED-seed figure a second time here, rcsl_policy_trainer.py:167,173: kept)
                if not normalized:
                    last_10_performance.append(ep_reward_mean)
                    self.logger.logkv("eval/episode_reward_no_fix_seed", rew2_mean)
                    self.logger.logkv("eval/episode_reward_std_no_fix_seed", rew2_std)
                else:
                    last_10_performance.append(norm_ep_rew_mean)
                    self.logger.logkv("eval/normalized_episode_reward_no_fix_seed", self.eval_env.get_normalized_score(rew2_mean) * 100)
                    self.logger.logkv("eval/normalized_episode_reward_std_no_fix_seed", self.eval_env.get_normalized_score(rew2_std) * 100)
                self.logger.logkv("eval/episode_length_no_fix_seed", len2_mean)
                self.logger.logkv("eval/episode_length_std_no_fix_seed", len2_std)
            self.logger.set_timestep(num_timesteps)
            self.logger.dumpkvs(exclude=["dynamics_training_progress"])
            torch.save(self.policy.state_dict(), os.path.join(self.logger.checkpoint_dir, "policy.pth"))
        self.logger.log("total time: {:.2f}s".format(time.time() - start_time))
        torch.save(self.policy.state_dict(), os.path.join(self.logger.model_dir, "policy.pth"))
        self.logger.close()
        return {"last_10_performance": np.mean(last_10_performance)}

    def _evaluate(self) -> Dict[str, List[float]]:
        self.eval_env.reset(seed=self.env_seed)      # fixed seed, every epoch (rcsl_policy_trainer.py:197)
        return self._rollout_eval(self.eval_env)

    def _evaluate_no_fix_seed(self) -> Dict[str, List[float]]:
        assert self.eval_env2 is not None
        return self._rollout_eval(self.eval_env2)

    def _rollout_eval(self, env) -> Dict[str, List[float]]:
        """the evaluation loop of ``_evaluate`` / ``_evaluate_no_fix_seed`` (rcsl_policy_trainer.py:199-276, 288-365)"""
        gymnasium = self.is_gymnasium_env

        def reset():
            if gymnasium:
                o, _ = env.reset()
                return env.get_true_observation(o)
            return env.reset()

        def step(action):
            if hasattr(env, "get_true_observation"):
                nxt, reward, terminal, _, _ = env.step(action.flatten())
            else:
                nxt, reward, terminal, _ = env.step(action.flatten())
            if gymnasium:
                nxt = env.get_true_observation(nxt)
            return nxt, reward, terminal

        def goal():
            return torch.tensor([[self.goal]]).type(torch.float32)

        self.policy.eval()
        obs = reset()
        done_eps = []
        episode_reward, episode_length = 0, 0
        if gymnasium:      # fixed-horizon episodes, the terminal flag is not consulted
            while len(done_eps) < self._eval_episodes:
                rtg = goal()
                for _ in range(self.horizon):
                    action = self.policy.select_action(obs.reshape(1, -1), rtg)
                    obs, reward, _ = step(action)
                    episode_reward += reward
                    rtg = rtg - reward
                    episode_length += 1
                done_eps.append({"episode_reward": episode_reward, "episode_length": episode_length})
                episode_reward, episode_length = 0, 0
                obs = reset()
        else:
            rtg = goal()
            while len(done_eps) < self._eval_episodes:
                action = self.policy.select_action(obs.reshape(1, -1), rtg)
                obs, reward, terminal = step(action)
                episode_reward += reward
                rtg = rtg - reward
                episode_length += 1
                if terminal:
                    done_eps.append({"episode_reward": episode_reward, "episode_length": episode_length})
                    episode_reward, episode_length = 0, 0
                    obs = reset()
                    rtg = goal()
        return {"eval/episode_reward": [d["episode_reward"] for d in done_eps],
                "eval/episode_length": [d["episode_length"] for d in done_eps]}

"""The bookkeeping of ``RcslPolicy.rollout`` (offlinerlkit/policy/rcsl.py: the loop body and the tail of ``rollout``) restated on arrays: what
a caller that already has each model step's transitions and verdicts must do to them.  The yardstick of the device trajectory store:
test_rcsl_rollout_cpu.py pins it to the reference's own rollout (tests/golden/ar_rollout.npz), test_gpu_rcsl_rollout.py compares
``orl_traj_*`` with it bit for bit."""
import numpy as np

KEYS = ["obss", "next_obss", "actions", "rewards", "terminals", "traj_idxs", "acc_rets", "rtgs"]


class HostBook:
    def __init__(self, n_traj):
        self.valid_idxs = np.arange(n_traj)          # trajectories still running
        self.returns = np.zeros(n_traj)              # float64, as the rollout keeps them
        self.acc_returns = np.zeros(n_traj)
        self.rows = {k: [] for k in KEYS[:-1]}
        self.rewards_arr = np.array([])
        self.num_transitions = 0

    def step(self, obs, act, next_obs, rew, term):
        """one model step: ``rew`` [n, 1] float32, ``term`` [n, 1] bool -> the mask of the rows that go on"""
        for k, v in zip(KEYS[:-1], (obs, next_obs, act, rew, term, self.valid_idxs, self.acc_returns)):
            self.rows[k].append(v)
        self.num_transitions += len(obs)
        self.rewards_arr = np.append(self.rewards_arr, rew.flatten())
        self.returns[self.valid_idxs] = self.returns[self.valid_idxs] + rew.flatten()
        self.acc_returns = self.acc_returns + rew.flatten()
        mask = (~term).flatten()
        if mask.sum() > 0:
            self.valid_idxs = self.valid_idxs[mask]
            self.acc_returns = self.acc_returns[mask]
        return mask

    def finish(self):
        out = {k: np.concatenate(v, axis=0) for k, v in self.rows.items()}
        out["rtgs"] = (self.returns[out["traj_idxs"]] - out["acc_rets"])[..., None]
        return out, {"num_transitions": self.num_transitions, "reward_mean": self.rewards_arr.mean(), "returns": self.returns}


def rollout(dynamics, rollout_policy, init_obss, rollout_length):
    """``rollout`` through ``HostBook``, for collaborators with the host interfaces (``select_action``, ``step``)"""
    book = HostBook(init_obss.shape[0])
    obs = init_obss
    frozen = hasattr(rollout_policy, "sample_init_noise")
    noise = rollout_policy.sample_init_noise(init_obss.shape[0]) if frozen else None
    for _ in range(rollout_length):
        act = rollout_policy.select_action(obs, noise)
        nxt, rew, term, _ = dynamics.step(obs, act)
        mask = book.step(obs, act, nxt, rew, term)
        if mask.sum() == 0:
            break
        obs = nxt[mask]
        if frozen:
            noise = noise[mask]
    return book.finish()


def bits(a):
    """the bit patterns of a float array (NaNs compare equal to themselves), other arrays as they are"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a

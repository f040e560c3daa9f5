"""The host side of the fused MBRCSL rollout (``orl_mbrcsl_rollout``) restated on a sequence of survivor counts: which steps are enqueued
and with which row bound, when the count of a step becomes known ``lag`` steps after the next one has been enqueued.  The yardstick of
test_rcsl_rollout_fused_cpu.py (the rule itself) and of test_gpu_rcsl_rollout_fused.py (``steps_enqueued``)."""


def enqueue_plan(n_traj, counts, lag):
    """``counts[t]``: the survivors of step t, had it run (non-increasing, <= n_traj); step t's live rows are ``n_traj`` for t = 0 and
    ``counts[t - 1]`` after.  Before step t the host knows ``counts[t - 1 - lag]`` at best.  -> [(t, bound_t)] of the steps enqueued"""
    plan, bound = [], int(n_traj)
    for t in range(len(counts)):
        k = t - 1 - int(lag)
        if k >= 0:
            bound = int(counts[k])
        if bound == 0:
            break
        plan.append((t, bound))
    return plan


def live_rows(n_traj, counts, t):
    return int(n_traj) if t == 0 else int(counts[t - 1])

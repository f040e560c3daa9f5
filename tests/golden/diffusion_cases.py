"""Inputs of the DiffusionBC fixtures (tests/golden/diffusion_*.npz), regenerated identically by the generator and by the tests; only
the reference's outputs are stored.  Everything comes from numpy's RandomState, so no torch version enters the inputs.

Shapes: obs_dim 5, act_dim 3 (not a multiple of 4), diffusion_step_embed_dim 16, kernel_size 5, batch 6 over an 8-row dataset (the
second batch of an epoch is 2 rows short), N = 10 diffusion iterations.  Case (a) has down_dims [8, 16, 32]: group sizes 1, 2 and 4
under GroupNorm(8); cases (b) and (c) share the two-level net [8, 16]; case (d), [24, 32], has no group of one channel."""
import numpy as np

OBS_DIM, ACT_DIM, DSED, KSIZE, NGROUPS, BATCH, NDATA, NITERS = 5, 3, 16, 5, 8, 6, 8, 10
CASES = {
    "a": dict(down_dims=[8, 16, 32], seed=101),
    "b": dict(down_dims=[8, 16], seed=202, steps=20),
    "c": dict(down_dims=[8, 16], seed=202, rows=4),
    # groups of 3 and 4 channels everywhere, so every tensor has a gradient (with 8 channels under GroupNorm(8) the final_conv norm
    # returns Mish(beta) and nothing upstream of it shows in the output): diffusion_d.npz, diffusion_d_traj.npz
    "d": dict(down_dims=[24, 32], seed=303, steps=12),
    # n_groups = 4 in the blocks (groups of 4 and 8 channels) while final_conv keeps GroupNorm(8) (2 channels per group): diffusion_e.npz
    "e": dict(down_dims=[16, 32], seed=404, n_groups=4),
}
for _c in CASES.values():
    _c.update(obs_dim=OBS_DIM, act_dim=ACT_DIM, dsed=DSED, kernel_size=KSIZE, B=BATCH, n=NDATA, N=NITERS)
    _c.setdefault("n_groups", NGROUPS)


def net_kwargs(c):
    return dict(diffusion_step_embed_dim=c["dsed"], down_dims=list(c["down_dims"]), kernel_size=c["kernel_size"], n_groups=c["n_groups"])


def make_params(c, shapes):
    """``shapes``: [(state_dict key, shape)] in state_dict order -> {key: float32 array}.  Linear / conv weights and biases
    U(-1, 1) / sqrt(fan_in) (every conv tap, the off-centre ones included), GroupNorm weights 1 + 0.3 U(-1, 1), GroupNorm biases
    0.3 U(-1, 1): no tensor is at a value that hides an error (gamma = 1, beta = 0)."""
    rng = np.random.RandomState(c["seed"])
    out = {}
    for key, shape in shapes:
        u = rng.uniform(-1.0, 1.0, size=shape)
        is_norm = ".block.1." in key
        if is_norm:
            v = (1.0 if key.endswith("weight") else 0.0) + 0.3 * u
        else:
            if key.endswith("weight"):
                fan_in = int(np.prod(shape[1:]))
                out["_fan_in"] = fan_in
            v = u / np.sqrt(out["_fan_in"])
        out[key] = v.astype(np.float32)
    out.pop("_fan_in", None)
    return out


def make_data(c):
    """the 8-row dataset: obs ~ N(0, 1), actions in [-1, 1]"""
    rng = np.random.RandomState(c["seed"] + 1)
    obs = rng.standard_normal((c["n"], c["obs_dim"])).astype(np.float32)
    act = np.tanh(rng.standard_normal((c["n"], c["act_dim"]))).astype(np.float32)
    return obs, act


def make_steps(c, steps):
    """teacher-forced draws of ``steps`` optimizer steps over shuffled epochs: per step (row indices, t, eps); an epoch is
    ceil(n / B) steps, the last one short"""
    rng = np.random.RandomState(c["seed"] + 2)
    out = []
    while len(out) < steps:
        perm = rng.permutation(c["n"])
        for s in range(0, c["n"], c["B"]):
            idx = perm[s:s + c["B"]].astype(np.int64)
            t = rng.randint(0, c["N"], size=len(idx)).astype(np.int64)
            eps = rng.standard_normal((len(idx), c["act_dim"])).astype(np.float32)
            out.append((idx, t, eps))
    return out[:steps]


def make_sample_inputs(c):
    """case (c): obs, init_noise [rows, 1, act_dim] and z [N, rows, act_dim]"""
    rng = np.random.RandomState(c["seed"] + 3)
    rows = c["rows"]
    obs = rng.standard_normal((rows, c["obs_dim"])).astype(np.float32)
    noise = rng.standard_normal((rows, 1, c["act_dim"])).astype(np.float32)
    z = rng.standard_normal((c["N"], rows, c["act_dim"])).astype(np.float32)
    return obs, noise, z

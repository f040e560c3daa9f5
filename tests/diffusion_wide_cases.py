"""DiffusionBC at the shapes it ships with -- wide GroupNorm groups, wide inputs, many rows, non-increasing down_dims: the cases, their
numpy references and the check functions of tests/test_gpu_diffusion_wide.py (tests/test_diffusion_wide_cpu.py proves both on the CPU).

Parameters, data and steps come from tests/golden/diffusion_cases.py (numpy RandomState only); nothing is stored.  Every batch has
t = 0 and t = N - 1 forced into its first two rows.

Bars.  D32 of a quantity is the distance of the fp32 numpy oracle from the float64 oracle on the same case (``helpers.scale_err`` for an
activation, ``diffusion_oracle.grad_distance`` for the gradients): what another fp32 evaluation of the same formulas loses.  An engine
value is held to 4 x D32 -- the 4 covers another summation order in the GEMMs and the group statistics, as in tests/test_gpu_diffusion.py
-- with the project's 1e-4 gate on pred, loss and sampled actions as the outer cap.  The loss cell, e0 and Adam / EMA are held to
4 x the first-order bound their float64 restatements carry (tests/row_refs.py).  No bar comes from an engine output."""
import functools

import numpy as np

import diffusion_cases as dc
import diffusion_oracle as orc
import row_refs as rr
from helpers import rel_err, scale_err

BAR = 4.0
GATE = 1e-4

_BASE = dict(obs_dim=5, act_dim=3, dsed=16, kernel_size=5, n_groups=8, B=6, n=8, N=10)
CASES = {
    "A": dict(n_groups=1, down_dims=[64, 65, 128], seed=1101),          # cg 64 exact, 65 partial, 128; concat offset 65; final cg 8
    "B": dict(n_groups=1, down_dims=[512], kernel_size=1, seed=1102),   # cg 512: all 8 slabs full; final cg 64
    "C": dict(n_groups=16, down_dims=[528], kernel_size=1, seed=1103),  # 16 waves, cg 33; final cg 66
    "D": dict(down_dims=[24, 32], dsed=256, act_dim=67, obs_dim=70, seed=1104),   # half 128; act / obs lane loops; 17 Philox quads
    "E": dict(down_dims=[24, 32], dsed=4, act_dim=1, obs_dim=1, seed=1105),       # half - 1 == 1; one action column
    "F": dict(down_dims=[24, 32], dsed=130, B=90, n=100, seed=1106),    # half 65; k_diff_loss loop; 90-row colsum; short batch of 10
    "G": dict(n_groups=16, down_dims=[528], kernel_size=1, B=2048, n=2048, seed=1107),   # CFG_BIG, wgrad K >= 1024, 2048-row colsum
    "H": dict(down_dims=[32, 16], n_groups=4, seed=1108),               # 4 gradient terms; identity residual on a concatenation
    "I": dict(down_dims=[24, 24, 24], n_groups=3, seed=1109),           # identity down_l.0 blocks (2 terms + a skip term)
}
CASES = {k: dict(_BASE, **v) for k, v in CASES.items()}
CASES["D100"] = dict(CASES["D"], N=100)                                  # for the e0 tap and the pred gate only
STEP_CASES = tuple("ABCDEFGHI")
SAMPLE_NET, SAMPLE_N = "C", 3


def legal(c):
    """the create-time rules of the engine (orl_diffusion_create), restated: None, or the refusal"""
    dims, G = c["down_dims"], c["n_groups"]
    if c["kernel_size"] < 1 or c["kernel_size"] % 2 == 0:
        return "kernel_size must be odd"
    if min(c["obs_dim"], c["act_dim"], c["B"], c["N"]) < 1:
        return "bad dims"
    if c["dsed"] < 4 or c["dsed"] % 2:
        return "step_embed_dim must be even and >= 4"
    if not 1 <= len(dims) <= 4:
        return "n_levels must be in [1, 4]"
    if not 1 <= G <= 16:
        return "n_groups must be in [1, 16]"
    for d in dims:
        if d < 1 or d % G:
            return "every channel count must be a multiple of n_groups"
        if d // G > 512:
            return "a group is wider than 512 channels"
    if dims[0] % orc.FINAL_GROUPS or dims[0] // orc.FINAL_GROUPS > 512:
        return "down_dims[0] must be a multiple of 8"
    return None


def group_widths(c):
    """channels per group of every GroupNorm of the net"""
    plan, _ = orc.block_plan(c["act_dim"], c["down_dims"])
    return sorted({p[2] // c["n_groups"] for p in plan} | {c["down_dims"][0] // orc.FINAL_GROUPS})


def shapes_of(c):
    from offlinerlkit.nets import ConditionalUnet1D
    net = ConditionalUnet1D(c["act_dim"], c["obs_dim"], **dc.net_kwargs(c))
    return [(k, tuple(v.shape)) for k, v in net.state_dict().items()]


def make_batches(c, steps):
    out = []
    for idx, t, eps in dc.make_steps(c, steps):
        t = t.copy()
        t[0], t[1] = 0, c["N"] - 1
        out.append((idx, t, eps))
    return out


def centre_taps(G):
    return {k: (v[:, :, v.shape[2] // 2] if v.ndim == 3 else v) for k, v in G.items()}


def stage_names(c):
    nb = len(orc.block_plan(c["act_dim"], c["down_dims"])[0])
    return ["gf", "mc", "film"] + [f"{s}.{b}" for b in range(nb) for s in ("y1", "out")] + ["yf", "pred"]


def run_oracle(P, c, data, batch, dtype, e0=None):
    """one teacher-forced batch through the numpy oracle -> {stage: array, "e0", "loss", "grads" (centre taps), "x_t", "eps"}"""
    obs, act = data
    idx, t, eps = batch
    loss, pred, G, xt, A = orc.loss_and_grads(P, c, act[idx], t, eps, obs[idx], dtype=dtype, e0=e0, keep=True)
    out = dict(e0=A["e0"], gf=A["gf"], mc=A["mc"], film=np.concatenate([b["film"] for b in A["blocks"]], axis=1), yf=A["yf"], pred=pred,
               loss=float(loss), grads=centre_taps(G), x_t=xt, eps=eps)
    for b, blk in enumerate(A["blocks"]):
        out[f"y1.{b}"], out[f"out.{b}"] = blk["y1"], A["outs"][b]
    return out


def distances(a, b, c):
    """the distance of ``a`` from the float64 result ``b`` per stage, and of the gradients"""
    d = {s: scale_err(a[s], b[s]) for s in stage_names(c)}
    d["grads"], d["noise"] = orc.grad_distance(a["grads"], b["grads"])
    return d


@functools.lru_cache(maxsize=None)
def reference(name):
    """per case, computed once: parameters, data, the batches (two for F: the second is its short one), and per batch the fp32 oracle,
    the float64 oracle and D32.  Read-only."""
    c = CASES[name]
    P = dc.make_params(c, shapes_of(c))
    data = dc.make_data(c)
    batches = make_batches(c, 2 if name == "F" else 1)
    o32 = [run_oracle(P, c, data, b, np.float32) for b in batches]
    o64 = [run_oracle(P, c, data, b, np.float64) for b in batches]
    return dict(c=c, P=P, data=data, batches=batches, o32=o32, o64=o64, D32=[distances(a, b, c) for a, b in zip(o32, o64)])


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def loss_ref(pred, eps):
    """k_diff_loss on given fp32 operands: mean((pred - eps)^2) by a 256-thread strided loop and a tree, times the rounded 1 / n"""
    d = rr.BV.exact(np.asarray(pred, np.float32)) - rr.BV.exact(np.asarray(eps, np.float32))
    n = d.v.size
    return rr.sum_((d * d).reshape(-1)) * rr.BV(1.0 / n, rr.U / n)


def check_e0(e0, t, dsed, tag, record=None):
    ref = orc.sinusoidal_ref(t, dsed)
    r = rr.ratio(np.asarray(e0).reshape(ref.shape), ref) / rr.FACTOR
    if record is not None:
        record[f"{tag} e0"] = r
    assert r <= 1.0, (tag, "e0: err / (4 x bound)", r)
    return r


def check_step(got, ref, D32, c, tag, record=None):
    """``got`` (an engine step, or an fp32 oracle) against the float64 oracle ``ref`` of the same batch: every stage and the gradients
    within BAR x D32, pred and loss inside the project's gate, the loss cell inside the bound of its own restatement on got's pred.
    Returns {stage: err / bar}; every ratio is recorded before anything is asserted."""
    ratios = {}
    for s in stage_names(c):
        assert D32[s] > 0.0, (tag, s)
        ratios[s] = scale_err(np.asarray(got[s]).reshape(ref[s].shape), ref[s]) / (BAR * D32[s])
    dg, noise = orc.grad_distance(got["grads"], ref["grads"])
    ratios["grads"] = dg / (BAR * D32["grads"])
    ratios["loss cell"] = rr.ratio(np.array(got["loss"]), loss_ref(got["pred"], got["eps"])) / rr.FACTOR
    gate_pred = scale_err(np.asarray(got["pred"]).reshape(ref["pred"].shape), ref["pred"])
    gate_loss = rel_err(np.array([got["loss"]]), np.array([ref["loss"]]), floor=1e-2)
    if record is not None:
        record.update({f"{tag} {k}": v for k, v in ratios.items()})
    worst = max(ratios, key=ratios.get)
    print(f"{tag}: worst err / bar {ratios[worst]:.3f} at {worst}; gradients {dg:.2e} (D32 {D32['grads']:.2e}); pred {gate_pred:.2e}, "
          f"loss {gate_loss:.2e} of the 1e-4 gate")
    assert noise == 0.0 and D32["noise"] == 0.0, (tag, "a tensor without a gradient", noise)
    assert sorted(got["grads"]) == sorted(ref["grads"])
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, "err / bar above 1", bad)
    assert gate_pred < GATE and gate_loss < GATE, (tag, gate_pred, gate_loss)
    return ratios


ADAM_STEPS = (0, 1, 2, 215443, 215444, 1000000)      # the EMA cap min(1 - (1 + s)^-0.75, 0.9999), s = k - 1, binds from k = 215444 on


def adam_blocks(n, seed):
    """random blocks of n floats: p, ema, exp_avg and exp_avg_sq (>= 0)"""
    rng = np.random.RandomState(seed)
    p, ema = (0.1 * rng.standard_normal(n)).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32)
    m = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    v = ((1e-3 * rng.standard_normal(n)) ** 2).astype(np.float32)
    return p, ema, m, v


def lr_table_for(k, lr=1e-4):
    """k + 1 entries, so that lr[k] is the last valid one; every other entry is half of it"""
    tab = np.full(k + 1, 0.5 * lr)
    tab[k] = lr
    return tab


def check_adam_ema(got, before, g, lr, k, tag, record=None):
    """the four blocks after one optimizer step (``got``: p, ema, m, v) against the restatement applied to the blocks before it and the
    gradient ``g``; 4 x its bound"""
    ref = orc.adam_ema_ref(*before, g, lr, k)
    ratios = {nm: rr.ratio(x, r) / rr.FACTOR for nm, x, r in zip(("params", "ema", "exp_avg", "exp_avg_sq"), got, ref)}
    if record is not None:
        record.update({f"{tag} k={k} {nm}": v for nm, v in ratios.items()})
    bad = {nm: v for nm, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, k, "err / (4 x bound) above 1", bad)
    return ratios


# ---- sampling -----------------------------------------------------------------------------------------------------------------------
def sample_case():
    return dict(CASES[SAMPLE_NET], N=SAMPLE_N)


def make_sample_inputs(c, rows):
    rng = np.random.RandomState(c["seed"] + 3)
    obs = rng.standard_normal((rows, c["obs_dim"])).astype(np.float32)
    noise = rng.standard_normal((rows, 1, c["act_dim"])).astype(np.float32)
    z = rng.standard_normal((c["N"], rows, c["act_dim"])).astype(np.float32)
    return obs, noise, z


@functools.lru_cache(maxsize=None)
def sample_reference(rows):
    """net C with N = 3: inputs, the fp32 and the float64 oracle's actions, D32 and the x0 values before the clip.  Read-only."""
    c = sample_case()
    P = dc.make_params(c, shapes_of(c))
    obs, noise, z = make_sample_inputs(c, rows)
    trace = []
    a64 = orc.sample(P, c, obs, noise, z, dtype=np.float64, trace=trace)
    a32 = orc.sample(P, c, obs, noise, z)
    return dict(c=c, P=P, obs=obs, noise=noise, z=z, a32=a32, a64=a64, D32=scale_err(a32, a64), x0=np.stack(trace))


def check_sample(got, ref64, D32, tag, record=None):
    """sampled actions against the float64 oracle's: BAR x D32, capped by the 1e-4 gate"""
    assert D32 > 0.0
    r = scale_err(got, ref64) / min(BAR * D32, GATE)
    if record is not None:
        record[tag] = r
    print(f"{tag}: scale_err {scale_err(got, ref64):.2e}, D32 {D32:.2e}, err / bar {r:.3f}")
    assert r <= 1.0, (tag, "err / bar", r)
    return r
